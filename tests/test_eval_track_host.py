"""The numpy definitions of the in-training evaluation (uavppo/eval_track.py), no GPU: reduce_chunk + summarise must equal
evaluate_with_lstm's _Episodes.end_chunk + .metrics on CPU tensors with no host-side rule, better_rule must play the table of
tests/_eval_track_cases.py, and check_eval must refuse bad keywords before any device is touched."""
import numpy as np
import pytest
import torch

import evaluate_with_lstm as ev
from _eval_track_cases import KINDS, RULE_FINAL_STATE, RULE_TABLE, records, sources
from uavppo import eval_track as et

F64 = torch.float64
DEV_RTOL = 4 * 2.0 ** -52          # room for a fused multiply-add inside torch.linalg.norm's reduction


def _torch_walk(chunks, start, src, limit, success_distance):
    """_Episodes over `chunks` = [(t0, flags, obs, pos)], the device stop rule's first hit read off bit3 of the records."""
    ep_steps, ep_state, ep_pos = start
    n = ep_steps.shape[0]
    ep = ev._Episodes(n, "cpu")
    ep.active = torch.from_numpy((ep_state & 1) == 0)
    ep.steps = torch.from_numpy(ep_steps.astype(np.int64))
    ep.stopped = torch.from_numpy((ep_state & 2) != 0)
    ep.final_pos = torch.from_numpy(ep_pos.copy())
    for t0, flags, obs, pos in chunks:
        k = flags.shape[1]
        f = torch.from_numpy(flags)
        stepped = (f & 4) == 0
        done_c = ((f & 1) != 0) & stepped
        rule = ((f & 8) != 0) & stepped
        at_thr = torch.where(rule, torch.arange(k)[None, :], k).amin(1)
        # a bit2 record holds NaN that end_chunk's gather may touch for envs it then masks out: give it numbers
        o, p = torch.nan_to_num(torch.from_numpy(obs)), torch.nan_to_num(torch.from_numpy(pos))
        ep.end_chunk(t0, k, done_c, o, p, k, at_thr)
        last_pos = p[:, k - 1]
    return ep, ep.metrics(torch.from_numpy(src), limit, last_pos, success_distance)


def _numpy_walk(chunks, start):
    st = start
    for t0, flags, obs, pos in chunks:
        st = et.reduce_chunk(flags, obs, pos, t0, *st)
    return st


def _compare(chunks, start, n, limit=300, sd=40.0):
    src = sources(n)
    ep, m = _torch_walk(chunks, start, src, limit, sd)
    steps, state, pos = _numpy_walk(chunks, start)
    out = et.summarise(steps, state, pos, src, limit, sd)
    ended = (state & 1) != 0
    assert np.array_equal(ended, ~ep.active.numpy())
    assert np.array_equal((state & 2) != 0, ep.stopped.numpy())
    assert np.array_equal(steps[ended], ep.steps.numpy()[ended])
    assert np.array_equal(pos[ended], ep.final_pos.numpy()[ended])                  # final_pos, exactly
    assert np.array_equal(out["steps"], m["steps"]) and np.array_equal(out["success"], m["success"])
    assert np.array_equal(out["stopped_early"], m["stopped_early"])
    rel = np.abs(out["deviation"] - m["deviations"]) / np.maximum(np.abs(m["deviations"]), 1e-300)
    assert rel.max() <= DEV_RTOL, rel.max()
    return steps, state, pos, out


@pytest.mark.parametrize("k", [1, 2, 9])
@pytest.mark.parametrize("D", [6, 8])
def test_reduce_and_summarise_equal_the_torch_bookkeeping(k, D):
    n = 8 * 11
    flags, obs, pos, start = records(n, k, D)
    steps, state, p, out = _compare([(50, flags, obs, pos)], start, n)
    kind = np.arange(n) % 8
    ended = (state & 1) != 0
    assert ended[kind == 0].all() and (steps[kind == 0] == 51).all(), KINDS[0]
    assert ended[kind == 1].all() and (steps[kind == 1] == 50 + k).all(), KINDS[1]
    assert not ended[kind == 2].any() and (out["steps"][kind == 2] == 300).all(), KINDS[2]
    assert np.array_equal(p[kind == 2], pos[kind == 2, k - 1].astype(np.float64))
    for kd in (3, 4, 5):
        assert ((state[kind == kd] & 3) == 3).all(), KINDS[kd]
    assert ((state[kind == 6] & 3) == 1).all(), KINDS[6]
    q = (np.arange(n) // 8) % k
    rows = np.arange(n)
    assert np.array_equal(p[kind == 3], pos[rows, q][kind == 3].astype(np.float64))                      # the rule alone: agent_pos
    assert np.array_equal(p[kind == 4], obs[rows, q][kind == 4][:, :2].astype(np.float64) * 500.0)     # with done: the terminal obs
    assert np.array_equal(p[kind == 5], pos[rows, q][kind == 5].astype(np.float64))                      # the first record counts
    assert (steps[kind == 5] == 50 + q[kind == 5] + 1).all()
    s0 = start
    assert np.array_equal(steps[kind == 7], s0[0][kind == 7]) and np.array_equal(state[kind == 7], s0[1][kind == 7])
    assert np.array_equal(p[kind == 7], s0[2][kind == 7]), KINDS[7]
    assert not np.isnan(p).any() and not np.isnan(out["sums"]).any()                # no bit2 record was read


def test_a_chunk_split_at_every_position_gives_the_unsplit_result():
    n, k, D = 8 * 11, 9, 6
    flags, obs, pos, start = records(n, k, D)
    whole = _numpy_walk([(20, flags, obs, pos)], start)
    for s in range(1, k):
        parts = [(20, flags[:, :s], obs[:, :s], pos[:, :s]), (20 + s, flags[:, s:], obs[:, s:], pos[:, s:])]
        got = _numpy_walk(parts, start)
        for a, b in zip(got, whole):
            assert a.dtype == b.dtype and np.array_equal(a, b), s
        _compare(parts, start, n)
    ones = _numpy_walk([(20 + i, flags[:, i:i + 1], obs[:, i:i + 1], pos[:, i:i + 1]) for i in range(k)], start)
    for a, b in zip(ones, whole):
        assert np.array_equal(a, b)


def test_summarise_sums_and_edge_cases():
    n = 600
    rng = np.random.default_rng(3)
    ep_steps = rng.integers(1, 300, n).astype(np.int32)
    ep_state = rng.integers(0, 4, n).astype(np.uint8)
    src = rng.uniform(0, 500, (n, 2))
    ep_pos = src + rng.normal(0, 30, (n, 2))
    ep_pos[5] = src[5] + np.array([24.0, 32.0])                    # a 3-4-5 offset: the deviation is 40 exactly
    out = et.summarise(ep_steps, ep_state, ep_pos, src, 300, 40.0, nan_count=0)
    assert out["deviation"][5] == 40.0 and out["success"][5]
    S = out["sums"]
    ok, ended = out["success"], (ep_state & 1) != 0
    assert S[0] == n and S[1] == ok.sum() and S[2] == out["steps"].sum() and S[6] == (~ended).sum() and S[7] == 0
    assert np.isclose(S[3], out["deviation"].sum(), rtol=1e-13) and np.isclose(S[4], (out["deviation"] ** 2).sum(), rtol=1e-13)
    assert np.isclose(S[5], out["deviation"][ok].sum(), rtol=1e-13)
    none = et.summarise(ep_steps, ep_state, src + 1000.0, src, 300, 40.0)
    assert none["sums"][1] == 0 and none["sums"][5] == 0.0          # no successes: 0, not the NaN of an empty mean
    cut = et.summarise(ep_steps, np.zeros(n, np.uint8), ep_pos, src, 123, 40.0, nan_count=4)
    assert cut["sums"][6] == n and (cut["steps"] == 123).all() and cut["sums"][2] == 123 * n and cut["sums"][7] == 4
    bad = ep_pos.copy()
    bad[17, 0] = np.nan
    nan = et.summarise(ep_steps, ep_state, bad, src, 300, 40.0)
    assert np.isnan(nan["deviation"][17]) and not nan["success"][17]
    assert np.isnan(nan["sums"][3]) and np.isnan(nan["sums"][4]) and not np.isnan(nan["sums"][5])    # the sums it enters, no other
    assert nan["sums"][1] == S[1] - int(ok[17])


def test_better_rule_plays_the_table():
    state = np.zeros(et.BEST_N)
    for it, sums, took, what in RULE_TABLE:
        state = et.better_rule(state, sums, it)
        assert state[6] == took, what
        if took:
            assert state[0] == sums[1] and state[1] == sums[2] and state[2] == it, what
    assert np.array_equal(state, RULE_FINAL_STATE)
    row = et.curve_row(6, RULE_TABLE[5][1], et.better_rule(np.zeros(et.BEST_N), RULE_TABLE[5][1], 6))
    assert len(row) == len(et.CURVE_COLUMNS) and row[0] == 6 and row[1] == 64 and row[2] == 6 / 64 and row[-1] == 1


@pytest.mark.parametrize("kw", [dict(eval_every=0), dict(eval_every=2.5), dict(eval_every=True), dict(eval_envs=0), dict(eval_envs="64"),
                                dict(eval_seed=-1), dict(eval_max_steps=0), dict(eval_chunk=0), dict(eval_chunk=1.5),
                                dict(eval_radius=0.0), dict(eval_radius=float("nan")), dict(keep_best=1)])
def test_check_eval_refuses_without_a_gpu(kw):
    with pytest.raises(ValueError, match=next(iter(kw))):
        et.check_eval(**{"eval_every": 2, **kw})
    from uavppo.trainer import VecPPOTrainer
    with pytest.raises(ValueError, match=next(iter(kw))):          # before any device is touched
        VecPPOTrainer(32, 16, "lstm", hidden=64, **{"eval_every": 2, **kw})


def test_check_eval_passes_the_defaults():
    c = et.check_eval()
    assert c["eval_every"] is None and c["eval_envs"] == 256 and c["eval_seed"] == 4321 and c["keep_best"] is True
    assert et.check_eval(5, 64, 1, 48, 16, 9.5, False) == dict(eval_every=5, eval_envs=64, eval_seed=1, eval_max_steps=48, eval_chunk=16,
                                                               eval_radius=9.5, keep_best=False)
