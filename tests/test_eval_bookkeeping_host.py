"""The host bookkeeping of evaluate_with_lstm.evaluate() on CPU tensors, no GPU: the fused path's one-call chunk reduction
(_Episodes.end_chunk over _StopRules.first_hits) must equal the loop body both paths share (_StopRules.step + _Episodes.end) walked
step by step over the same chunk, and the `max_steps` tail must close the episodes that never ended."""
import itertools

import pytest
import torch

import evaluate_with_lstm as ev

K = 3                                                   # steps per chunk; an index of K means "not in this chunk"
F64 = torch.float64


class _Predictor:                                       # what _DevicePeakStop reads off a PeakAndStopPredictor
    class lstm:
        hidden_size, num_layers, input_size = 32, 1, 1

    def flat_params(self):
        return torch.zeros(1)


class _Controller:                                      # what _DeviceThreshold reads off a ThresholdController
    model, lo, scale, window_size, min_activate_steps = None, 0.0, 1.0, 10, 20

    def reset(self):
        pass


def _chunk():
    """128 envs: every (at_done, at_peak, at_thr) in {0 .. K}^3, once active and once already inactive, with records that tell
    every (env, step) apart.  A rule fires at its index and at every later step of the chunk; done is one record."""
    idx = torch.tensor(list(itertools.product(range(K + 1), repeat=3)) * 2)
    at_done, at_peak, at_thr = idx[:, 0], idx[:, 1], idx[:, 2]
    N = idx.shape[0]
    e, i = torch.arange(N)[:, None], torch.arange(K)[None, :]
    obs = torch.zeros(N, K, 6)
    obs[:, :, 0], obs[:, :, 1], obs[:, :, 2] = (8 * e + 2 * i + 1) / 4096.0, (8 * e + 2 * i + 2) / 4096.0, (e + i) / 1024.0
    pos = torch.stack([1000.0 + 8 * e + 2 * i, 1000.5 + 8 * e + 2 * i], 2)
    peak_c = (5000.0 + 4 * e + i).to(torch.float32)
    prob_c = torch.where(i >= at_peak[:, None], 0.9, torch.where(e % 2 == 0, 0.1, float("nan"))).to(torch.float32)
    stop_c = (i >= at_thr[:, None]).to(torch.uint8)
    done_c = i == at_done[:, None]
    hit = lambda at: torch.where(at < K, at, -1).to(torch.int32)
    return N, at_done, at_peak, at_thr, done_c, obs, pos, peak_c, prob_c, stop_c, hit(at_peak), hit(at_thr)


def _start(N):
    """(_Episodes, peak_pred): the second half of the envs ended earlier and holds results that nothing may touch."""
    ep = ev._Episodes(N, "cpu")
    half = N // 2
    ep.active[half:] = False
    ep.steps[half:] = 7
    ep.stopped[half::2] = True
    ep.final_pos[half:] = torch.arange(2 * half, dtype=F64).reshape(half, 2) - 99.0
    peak_pred = torch.full((N,), float("nan"), dtype=F64)
    peak_pred[half::3] = 3.5
    return ep, peak_pred


def _same(a, b):
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


@pytest.mark.parametrize("t0", [0, 50])
def test_chunk_reduction_equals_the_step_by_step_walk(t0):
    N, at_done, at_peak, at_thr, done_c, obs, pos, peak_c, prob_c, stop_c, peak_hit, thr_hit = _chunk()
    assert N == 128
    for name, m in (("done and hit on the same step", (at_done == at_peak) & (at_done < K)),
                    ("both rules on the same step", (at_peak == at_thr) & (at_peak < K)),
                    ("a hit after done", (at_done < at_peak) & (at_peak < K)),
                    ("nothing in the chunk", (at_done == K) & (at_peak == K) & (at_thr == K))):
        assert m[:64].any() and m[64:].any(), name

    rules = ev._StopRules(_Controller(), _Predictor(), 20, N, "cpu", True, True)
    assert not rules.replay
    rules.dps.scan = lambda series, active: (peak_hit, peak_c, prob_c)
    rules.dth.scan = lambda series, active, t0, want_steps: (thr_hit, stop_c, None)
    conc = obs[:, :, 2]

    # the loop body, step by step
    walk, rules.peak_pred = _start(N)
    rules.scan(conc, walk.active, t0, True)
    for i in range(K):
        done_b = done_c[:, i]
        pos_end = torch.where(done_b[:, None], obs[:, i, :2].to(F64) * 500.0, pos[:, i].to(F64))
        stop_now = rules.step(i, t0 + i + 1, conc[:, i], walk.active)
        assert torch.equal(stop_now, (i >= at_peak) | (i >= at_thr))
        walk.end(walk.active & (done_b | stop_now), t0 + i + 1, stop_now, pos_end)
    walked_pred = rules.peak_pred

    # the same chunk in one call
    ep, pred0 = _start(N)
    got_peak, got_thr = rules.first_hits(K)
    assert torch.equal(got_peak, at_peak) and torch.equal(got_thr, at_thr)
    pred = ep.end_chunk(t0, K, done_c, obs, pos, got_peak, got_thr, peak_c, pred0)
    for name in ("steps", "stopped", "final_pos", "active"):
        assert torch.equal(getattr(ep, name), getattr(walk, name)), name
    assert _same(pred, walked_pred)

    # what must have happened, from the indices alone
    first = torch.minimum(at_done, torch.minimum(at_peak, at_thr))
    was = _start(N)[0]
    ends = was.active & (first < K)
    assert torch.equal(ep.active, was.active & ~ends) and torch.equal(ep.steps[ends], first[ends] + t0 + 1)
    assert torch.equal(ep.steps[~ends], was.steps[~ends]) and torch.equal(ep.final_pos[~ends], was.final_pos[~ends])
    assert torch.equal(ep.stopped, was.stopped | (ends & (torch.minimum(at_peak, at_thr) == first)))
    assert _same(pred[~ends], pred0[~ends]) and torch.isnan(pred[ends & (at_peak > first)]).all()
    by_peak = ends & (at_peak == first)
    assert torch.equal(pred[by_peak], (5000.0 + 4 * torch.arange(N) + first)[by_peak].to(F64))

    # a rule that is not there is the plain int K
    for rows, ints in ((at_peak == K, (K, at_thr)), (at_thr == K, (at_peak, K)), ((at_peak == K) & (at_thr == K), (K, K))):
        a, b = _start(N)[0], _start(N)[0]
        a.active &= rows
        b.active &= rows
        assert a.active.sum() == rows[:64].sum() > 0
        pa = a.end_chunk(t0, K, done_c, obs, pos, *ints, peak_c, pred0)
        pb = b.end_chunk(t0, K, done_c, obs, pos, at_peak, at_thr, peak_c, pred0)
        for name in ("steps", "stopped", "final_pos", "active"):
            assert torch.equal(getattr(a, name), getattr(b, name)), name
        assert _same(pa, pb)
    assert _start(N)[0].end_chunk(t0, K, done_c, obs, pos, K, K) is None


def test_max_steps_tail_closes_the_episodes_still_active():
    ep = ev._Episodes(4, "cpu")
    src = torch.tensor([[0.0, 0.0], [10.0, 0.0], [0.0, 0.0], [3.0, 4.0]], dtype=F64)
    ep.end(torch.tensor([True, False, False, False]), 5, torch.tensor([True, True, False, False]),
           torch.tensor([[3.0, 4.0]] * 4, dtype=F64))
    ep.end(torch.tensor([False, False, True, False]), torch.tensor([0, 0, 9, 0]), torch.zeros(4, dtype=torch.bool),
           torch.tensor([[0.0, 30.0]] * 4, dtype=F64))
    assert ep.active.tolist() == [False, True, False, True]
    last_pos = torch.tensor([[100.0, 100.0], [10.0, 12.0], [100.0, 100.0], [3.0, 4.0]])      # f32, as the records' agent_pos
    out = ep.metrics(src, 300, last_pos, 20.0)
    assert out["steps"].tolist() == [5, 300, 9, 300] and out["steps"].dtype.name == "int64"
    assert out["deviations"].tolist() == [5.0, 12.0, 30.0, 0.0] and out["deviations"].dtype.name == "float64"
    assert out["success"].tolist() == [True, True, False, True] and out["stopped_early"].tolist() == [True, False, False, False]
    assert "peak_pred" not in out and ep.active.tolist() == [False, True, False, True]
