"""CPU: the restated stop rule and episode bookkeeping of PPOV1.1/evaluate_model.py (tests/_eval_v11_check.py) against values
recorded from the reference's own ModelEvaluator (tests/golden/eval_v11.npz, eval_v11_results.csv; tools/gen_golden_eval_v11.py),
against numpy's np.std itself, and the CSV writer of the product's evaluate_model.py against the reference's CSV text."""
import os

import numpy as np
import pytest

import _eval_v11_check as ck
from conftest import GOLDEN

F = np.float32


@pytest.fixture(scope="module")
def g():
    d = np.load(os.path.join(GOLDEN, "eval_v11.npz"), allow_pickle=False)
    return {k: d[k] for k in d.files}


def _episodes(g):
    ends = np.cumsum(g["ep_len"])
    for i, (a, b) in enumerate(zip(ends - g["ep_len"], ends)):
        yield i, slice(int(a), int(b))


def _bits(x):
    return np.asarray(x, F).view(np.uint32)


def test_fixture_holds_the_cases_the_rule_needs(g):
    assert int(g["window"]) == ck.WINDOW == 10 and float(g["stability_threshold"]) == ck.POS_STD_MAX
    assert float(g["conc_threshold"]) == ck.CONC_MIN and float(g["conc_peak"]) == ck.CONC_PEAK
    cap = int(g["step_cap"])
    last_stop = np.array([bool(g["stop"][s][-1]) for _, s in _episodes(g)])
    steps = g["steps"]
    assert len(steps) >= 18
    assert (last_stop & (steps == 10)).any(), "no stop at exactly step 10"
    assert (last_stop & (steps > 10)).any(), "no stop later than step 10"
    assert (~last_stop & (steps == cap)).any(), "no episode that runs to the cap without stopping"
    full = ~np.isnan(g["pos_std"])
    stable = full & (g["pos_std"] < F(ck.POS_STD_MAX))
    high = np.array([ck.conc_high(o)[0] for o in g["obs2"]])
    assert (stable & ~high).any(), "no step with the stability half true and the concentration half false"
    assert (~stable & full & high).any(), "no step with only the concentration half true"
    # a stop decision anywhere but on an episode's last step would have ended the episode there
    for _, s in _episodes(g):
        assert not g["stop"][s][:-1].any()


def test_rule_reproduces_every_recorded_value_and_decision(g):
    n_val = 0
    for _, s in _episodes(g):
        pos, obs2 = g["pos"][s], g["obs2"][s]
        for t in range(len(pos)):
            stop, v = ck.rule(list(pos[:t + 1]), obs2[t])
            want = g["pos_std"][s][t]
            if t + 1 < ck.WINDOW:
                assert np.isnan(v) and np.isnan(want)
            else:
                assert _bits(v) == _bits(want), (t, float(v), float(want))
                n_val += 1
            assert stop == bool(g["stop"][s][t]), t
    assert n_val > 2000


def test_bookkeeping_reproduces_the_reference_rows(g):
    cap, radius = int(g["step_cap"]), float(g["radius"])
    for i, s in _episodes(g):
        steps, dev, ok, conc, fired, vals, stops = ck.episode_results(g["pos"][s], g["obs2"][s], g["done"][s], g["source_pos"][i],
                                                                     radius, cap)
        assert steps == int(g["steps"][i]) == int(g["ep_len"][i])
        assert abs(dev - float(g["deviation"][i])) <= 1e-12
        assert ok == bool(g["success"][i])
        assert _bits(conc) == _bits(g["final_conc"][i])
        assert fired == bool(g["stop"][s][-1])
        assert np.array_equal(stops, g["stop"][s])
        assert np.array_equal(_bits(vals), _bits(g["pos_std"][s]))
        # truncated streams behave like the loop too: a lower cap ends the episode at the cap
        if steps > 12:
            assert ck.episode_results(g["pos"][s], g["obs2"][s], g["done"][s], g["source_pos"][i], radius, 12)[0] == 12


def test_restatement_equals_numpy_std_bit_for_bit():
    rng = np.random.default_rng(0)
    n = near = 0
    for k in range(12000):
        if k % 3 == 0:            # wide: anywhere on the field
            w = (rng.random((10, 2)) * 500).astype(F)
        elif k % 3 == 1:          # a settled agent: small spread around a point, std of the order of the threshold
            w = (rng.random(2) * 500 + rng.standard_normal((10, 2)) * rng.uniform(0.5, 4.0)).astype(F)
        else:                     # scaled so that the value lies within 1e-3 of 2.0
            w = rng.random(2) * 480 + 10 + rng.standard_normal((10, 2))
            w = w.mean(0) + (w - w.mean(0)) * ((2.0 + rng.uniform(-9e-4, 9e-4)) / np.std(w, axis=0).mean())
            w = w.astype(F)
        ref = np.std([r for r in w], axis=0).mean()            # the reference's expression over a list of f32 pairs
        assert ref.dtype == F
        assert _bits(ck.pos_std(w)) == _bits(ref), (k, w)
        n += 1
        near += abs(float(ref) - 2.0) < 1e-3
    assert n >= 10000 and near >= 1000, (n, near)
    # degenerate windows: a stuck agent, a window that moves along one coordinate only
    for v in (499.999, 0.0, 137.25):                           # (the rounded mean of ten equal values need not be the value)
        w = np.full((10, 2), v, F)
        assert _bits(ck.pos_std(w)) == _bits(np.std([r for r in w], axis=0).mean())
    w = np.zeros((10, 2), F)
    w[:, 0] = np.arange(10) * 25
    assert _bits(ck.pos_std(w)) == _bits(np.std(w, axis=0).mean())


def test_csv_writer_reproduces_the_reference_csv(g, tmp_path):
    import evaluate_model as em
    p = tmp_path / "evaluation_results.csv"
    em.write_results_csv(str(p), g["steps"], g["deviation"], g["success"], g["final_conc"])
    want = open(os.path.join(GOLDEN, "eval_v11_results.csv"), "rb").read()
    assert p.read_bytes() == want
    assert want.splitlines()[0] == b"episode,steps,deviation,success,final_conc"
