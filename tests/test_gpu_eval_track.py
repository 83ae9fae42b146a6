"""csrc/eval_track.hip against the numpy definitions of uavppo/eval_track.py, bit for bit: uav_greedy_reduce (integers and f64
positions), uav_greedy_summary (per-env outputs and all eight sums), uav_keep_best (state and best).  Synthetic records only
(tests/_eval_track_cases.py); the trainer-level tests are in tests/test_gpu_eval_trainer.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from _eval_track_cases import RULE_FINAL_STATE, RULE_TABLE, records, sources

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    from uavppo import ops as o
    return o


@pytest.fixture(scope="module")
def et():
    from uavppo import eval_track
    return eval_track


def bits64(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _reduce(ops, chunks, start):
    """uav_greedy_reduce over chunks = [(t0, flags, obs, pos)] from the start state -> numpy (ep_steps, ep_state, ep_pos)"""
    st = [dev(a.copy()) for a in start]
    for t0, flags, obs, pos in chunks:
        ops.greedy_reduce({"flags": dev(flags), "obs": dev(obs), "pos": dev(pos)}, t0, *st)
    return [t.cpu().numpy() for t in st]


def _same_state(got, want):
    return (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[0].dtype == np.int32 and got[1].dtype == np.uint8
            and np.array_equal(bits64(got[2]), bits64(want[2])))


@pytest.mark.parametrize("D", [6, 8])
@pytest.mark.parametrize("k", [1, 2, 63, 64, 65, 250])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_greedy_reduce_is_reduce_chunk(ops, et, n, k, D):
    """Every case kind of records() (an end at record 0, at k - 1, nowhere; bit3 alone, with bit0, before bit0; bit2 records after
    an end; envs that come in ended with sentinels), NaN in the obs / pos of every bit2 record."""
    flags, obs, pos, start = records(n, k, D)
    assert np.isnan(obs[(flags & 4) != 0]).all()
    want = et.reduce_chunk(flags, obs, pos, 37, *start)
    got = _reduce(ops, [(37, flags, obs, pos)], start)
    assert _same_state(got, want)
    assert not np.isnan(got[2]).any()                                   # no bit2 record was read


@pytest.mark.parametrize("n,k", [(65, 9), (257, 65)])
def test_greedy_reduce_chunk_split_invariance(ops, et, n, k):
    flags, obs, pos, start = records(n, k, 6)
    whole = _reduce(ops, [(20, flags, obs, pos)], start)
    assert _same_state(whole, et.reduce_chunk(flags, obs, pos, 20, *start))
    for s in (range(1, k) if k < 10 else (1, 31, 63, 64)):
        parts = [(20, flags[:, :s], obs[:, :s], pos[:, :s]), (20 + s, flags[:, s:], obs[:, s:], pos[:, s:])]
        assert _same_state(_reduce(ops, parts, start), whole), s
    if k < 10:
        ones = [(20 + i, flags[:, i:i + 1], obs[:, i:i + 1], pos[:, i:i + 1]) for i in range(k)]
        assert _same_state(_reduce(ops, ones, start), whole)


def _summary(ops, ep_steps, ep_state, ep_pos, src, limit, sd, nan_count=None, per_env=True):
    n = ep_steps.shape[0]
    sums = torch.full((ops.EVAL_SUM_N,), -7.0, dtype=torch.float64, device=DEV)
    out = {}
    if per_env:
        out = {"deviation": torch.zeros(n, dtype=torch.float64, device=DEV), "steps": torch.zeros(n, dtype=torch.int32, device=DEV),
               "success": torch.zeros(n, dtype=torch.uint8, device=DEV)}
    nc = None if nan_count is None else torch.tensor([nan_count], dtype=torch.int32, device=DEV)
    ops.greedy_summary(dev(ep_steps), dev(ep_state), dev(ep_pos), dev(src), limit, sd, sums, nan_count=nc, **out)
    return sums.cpu().numpy(), {k: v.cpu().numpy() for k, v in out.items()}


def _episodes(n, seed):
    rng = np.random.default_rng(seed)
    ep_steps = rng.integers(1, 300, n).astype(np.int32)
    ep_state = rng.integers(0, 4, n).astype(np.uint8)
    src = rng.uniform(0, 500, (n, 2))
    ep_pos = src + rng.normal(0, 30, (n, 2))
    return ep_steps, ep_state, ep_pos, src


def _check_summary(ops, et, ep_steps, ep_state, ep_pos, src, limit, sd, nan_count=None):
    want = et.summarise(ep_steps, ep_state, ep_pos, src, limit, sd, nan_count or 0)
    sums, env = _summary(ops, ep_steps, ep_state, ep_pos, src, limit, sd, nan_count)
    assert np.array_equal(bits64(sums), bits64(want["sums"])), (sums, want["sums"])
    assert np.array_equal(bits64(env["deviation"]), bits64(want["deviation"]))
    assert np.array_equal(env["steps"], want["steps"]) and np.array_equal(env["success"] != 0, want["success"])
    sums2, _ = _summary(ops, ep_steps, ep_state, ep_pos, src, limit, sd, nan_count, per_env=False)      # the outputs are optional
    assert np.array_equal(bits64(sums2), bits64(sums))
    return want


@pytest.mark.parametrize("n", [1, 63, 255, 256, 257, 1024, 4097])
def test_greedy_summary_is_summarise(ops, et, n):
    ep_steps, ep_state, ep_pos, src = _episodes(n, n)
    if n > 5:
        ep_pos[5] = src[5] + np.array([24.0, 32.0])                     # 3-4-5: the deviation equals success_distance exactly
    want = _check_summary(ops, et, ep_steps, ep_state, ep_pos, src, 300, 40.0, nan_count=0)
    if n > 5:
        assert want["deviation"][5] == 40.0 and want["success"][5]
    assert want["sums"][0] == n and (n == 1 or 0 < want["sums"][1] < n)


def test_greedy_summary_edge_cases(ops, et):
    n = 300
    ep_steps, ep_state, ep_pos, src = _episodes(n, 9)
    cut = _check_summary(ops, et, ep_steps, np.zeros(n, np.uint8), ep_pos, src, 123, 40.0, nan_count=4)      # all cut off
    assert cut["sums"][6] == n and cut["sums"][2] == 123 * n and cut["sums"][7] == 4
    none = _check_summary(ops, et, ep_steps, ep_state, src + 1000.0, src, 300, 40.0)                          # no successes
    assert none["sums"][1] == 0 and none["sums"][5] == 0.0
    bad = ep_pos.copy()
    bad[17, 1] = np.nan                                                                                          # a NaN position
    nan = _check_summary(ops, et, ep_steps, ep_state, bad, src, 300, 40.0)
    assert np.isnan(nan["deviation"][17]) and not nan["success"][17] and np.isnan(nan["sums"][3]) and not np.isnan(nan["sums"][5])


@pytest.mark.parametrize("n_params", [1, 255, 256, 257, 36230])
def test_keep_best_plays_the_rule_table(ops, et, n_params):
    state = torch.zeros(ops.BEST_N, dtype=torch.float64, device=DEV)
    sentinel = torch.full((n_params,), float("nan"), device=DEV).view(torch.int32).fill_(0x7FC12345).view(torch.float32)
    best = sentinel.clone()
    want_state, want_best = np.zeros(ops.BEST_N), best.view(torch.int32).cpu().numpy().copy()
    for it, sums, took, what in RULE_TABLE:
        cand = (torch.arange(n_params, device=DEV, dtype=torch.float32) + 1000.0 * it).contiguous()
        ops.keep_best(state, dev(sums), it, cand, best)
        want_state = et.better_rule(want_state, sums, it)
        assert want_state[6] == took, what
        if took:
            want_best = cand.view(torch.int32).cpu().numpy().copy()
        assert np.array_equal(bits64(state.cpu().numpy()), bits64(want_state)), what
        assert np.array_equal(best.view(torch.int32).cpu().numpy(), want_best), what      # a non-improving call leaves every bit
    assert np.array_equal(want_state, RULE_FINAL_STATE)


def test_the_entry_points_refuse_with_a_reason(ops):
    from uavppo import _lib
    lib, h = _lib.lib(), ops.Context.get(torch.device(DEV)).handle
    a = torch.zeros(64, dtype=torch.float64, device=DEV)
    p = C.c_void_p(a.data_ptr())
    for args, what in (((None, p, p, 1, 1, 6, 0, p, p, p), b"NULL"), ((p, p, p, 0, 1, 6, 0, p, p, p), b"at least 1"),
                       ((p, p, p, 1, 0, 6, 0, p, p, p), b"at least 1"), ((p, p, p, 1, 1, 1, 0, p, p, p), b"at least 2"),
                       ((p, p, p, 1 << 12, 1 << 12, 128, 0, p, p, p), b"2^31")):
        assert lib.uav_greedy_reduce(h, *args, None) == 2 and what in lib.uav_last_error(), what
    assert lib.uav_greedy_summary(h, p, p, p, p, 0, 5, 40.0, None, None, None, None, p, None) == 2
    assert lib.uav_greedy_summary(h, p, p, p, p, 1, 5, 40.0, None, None, None, None, None, None) == 2 and b"NULL" in lib.uav_last_error()
    assert lib.uav_keep_best(h, p, p, 1, p, p, 4, None) == 2 and b"same buffer" in lib.uav_last_error()
    assert lib.uav_keep_best(h, p, p, 1, p, None, 4, None) == 2 and b"NULL" in lib.uav_last_error()
