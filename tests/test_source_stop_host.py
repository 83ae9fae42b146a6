"""CPU: the numpy statement of the estimator's stop rule (uavppo/source_stop.py).  stop_rule against a plain per-record loop,
stop_scan_chunk against the sequential definition (accumulate record by record, solve after each), the marked flags through
moments_chunk / reduce_chunk, the refusals, and the margin property of the inputs tests/test_gpu_source_stop.py relies on.  The
kernel is tested against this statement there."""
import numpy as np
import pytest

from _source_stop_cases import SHAPES, SPLIT_SHAPES, SPLITS, TKE_OFF, case_sets, drive, margins, placed_hits, start_state, walkers

EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def sf():
    from uavppo import source_fit
    return source_fit


@pytest.fixture(scope="module")
def ss():
    from uavppo import source_stop
    return source_stop


def bits64(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def _loop_rule(mu, status, pos, t0, rs, cfg):
    """The rule as a plain loop over one env's records; python floats are f64."""
    pmx, pmy, pfit, run, hit_step, hx, hy = (float(v) for v in rs)
    first = -1
    if hit_step > 0.0:
        return first, [pmx, pmy, pfit, run, hit_step, hx, hy]
    tol2, near2 = float(cfg["settle_tol"]) * float(cfg["settle_tol"]), float(cfg["near"]) * float(cfg["near"])
    for i in range(len(status)):
        if status[i] == 255:
            continue
        fit = status[i] == 0
        mx, my = (float(mu[i, 0]), float(mu[i, 1])) if fit else (0.0, 0.0)
        dx, dy = mx - pmx, my - pmy
        settled = fit and pfit != 0.0 and dx * dx + dy * dy <= tol2
        run = run + 1.0 if settled else 0.0
        nx, ny = float(pos[i, 0]) - mx, float(pos[i, 1]) - my
        pmx, pmy, pfit = mx, my, 1.0 if fit else 0.0
        if fit and run >= cfg["patience"] and nx * nx + ny * ny <= near2 and t0 + i + 1 >= cfg["min_steps"]:
            return i, [pmx, pmy, pfit, run, float(t0 + i + 1), mx, my]
    return first, [pmx, pmy, pfit, run, hit_step, hx, hy]


def _random_estimates(n, k, seed):
    """Estimates that move by about settle_tol, statuses of every kind, runs of FITTED records long enough to cross 63 | 64."""
    rng = np.random.default_rng(seed)
    mu = np.cumsum(rng.normal(0.0, 0.3, (n, k, 2)), 1) + 200.0
    status = rng.choice(np.array([0, 0, 0, 0, 0, 0, 0, 1, 2, 3, 255], np.uint8), (n, k))
    status[: n // 2] = np.where(rng.uniform(size=(n // 2, k)) < 0.01, 255, 0)           # long runs
    mu[: n // 4] = np.round(mu[: n // 4] * 0.02) / 0.02                                  # and long settled ones
    mu = np.where((status == 0)[:, :, None], mu, np.nan)
    pos = (mu + rng.normal(0.0, 20.0, (n, k, 2))).astype(np.float32)
    pos[status == 255] = np.nan
    return mu, status, pos


@pytest.mark.parametrize("cfg", [dict(), dict(patience=1), dict(patience=60, settle_tol=2.0), dict(near=25.0), dict(min_steps=70, near=40.0),
                                 dict(settle_tol=0.0, patience=2)])
def test_stop_rule_is_the_plain_loop(ss, cfg):
    """Exact equality of first_hit and of every bit of the rule state, over one chunk and over chunks cut at 63 | 64 | 65 and 1."""
    cfg = ss.check_source_stop(**cfg)
    n, k = 48, 200
    mu, status, pos = _random_estimates(n, k, 5)
    hits = 0
    for cuts in ([0, k], [0, 63, k], [0, 64, 128, k], [0, 65, k], [0, 1, 2, k]):
        rs = np.zeros((n, 7))
        want = [list(r) for r in rs]
        for a, b in zip(cuts[:-1], cuts[1:]):
            fh, rs = ss.stop_rule(mu[:, a:b], status[:, a:b], pos[:, a:b], a, rs, cfg)
            for e in range(n):
                w, want[e] = _loop_rule(mu[e, a:b], status[e, a:b], pos[e, a:b], a, want[e], cfg)
                assert fh[e] == w, (e, a, fh[e], w)
            assert np.array_equal(bits64(rs), bits64(np.array(want)))
            hits += int((fh >= 0).sum())
    if cfg["patience"] <= 3:
        assert hits > n
    if cfg["patience"] == 60:
        assert hits > 0                                                                 # a run that crossed 63 | 64


def _sequential(sf, ss, ep, fit_cfg):
    """The definition: per env the used records' contributions added one after the other in time order (np.cumsum), solve after
    each eligible record -> (eligible, count, centre, moments [n, k, 14], sum of |terms| [n, k, 14], the systems, est, status) over
    the whole chunk, however the statement is driven over its pieces."""
    n, k = ep["flags"].shape
    take = ss.eligible_records(ep["flags"], ep["ended"])
    used, b, cell = sf.used_records(ep["flags"], ep["obs"], ep["pos"], ep["ended"], fit_cfg["use_tke"], fit_cfg["background"],
                                    fit_cfg["floor"])
    e = np.arange(n)
    i0 = used.argmax(1)
    cx = np.where(used.any(1), cell[e, i0, 0], 0).astype(np.float64)
    cy = np.where(used.any(1), cell[e, i0, 1], 0).astype(np.float64)
    p, q = (cell[:, :, 0] - cx[:, None]) / 32.0, (cell[:, :, 1] - cy[:, None]) / 32.0
    r = p * p + q * q
    bu = np.where(used, b, 1.0)
    w, lb = bu * bu, np.log(bu)
    phi = [np.ones_like(p), p, q, r]
    terms = [w * phi[i] * phi[j] for i in range(4) for j in range(i, 4)] + [w * phi[i] * lb for i in range(4)]
    terms = np.where(used[:, :, None], np.stack(terms, 2), 0.0)
    mom, mag = np.cumsum(terms, 1), np.cumsum(np.abs(terms), 1)
    count = np.cumsum(used, 1).astype(np.float64)
    sys = np.zeros((n, k, 20))
    sys[:, :, 0], sys[:, :, 1], sys[:, :, 2], sys[:, :, 3:17] = count, cx[:, None], cy[:, None], mom
    est, status = sf.solve(sys.reshape(-1, 20), fit_cfg["min_samples"], fit_cfg["min_pivot"])
    status = np.where(take, status.reshape(n, k), 255)
    return take, count, cx, cy, mom, mag, sys, est.reshape(n, k, 8), status


@pytest.mark.parametrize("shape", [(96, 130, 6, 0)] + SPLIT_SHAPES)
def test_stop_scan_chunk_is_the_sequential_definition(sf, ss, shape):
    """With a rule that cannot fire: counts, centres and statuses equal; every moment within the rounding of a reordered sum of
    that many terms, (count + 4) 2^-52 sum |terms|; the scaled coefficients u = a d norm-wise within 64 eps cond(S) of the
    sequential ones, the bound of solve against lstsq in tests/test_source_fit_host.py (the largest fraction of it is printed)."""
    worst = 0.0
    n, k, D, seed = shape
    cannot = ss.check_source_stop(patience=1 << 30)
    for name, ep, kw in case_sets(n, k, D, seed):
        fit_cfg = sf.check_source_fit(**kw)
        for s in (None,) + (SPLITS if shape in SPLIT_SHAPES else ()):
            cuts = [0, k] if s is None else [0, s, k]
            take, count, cx, cy, mom, mag, sys, est, status = _sequential(sf, ss, ep, fit_cfg)
            st, outs = drive(ss, ep, fit_cfg, cannot, cuts)
            got_status, got_sys = [o["status_steps"] for o in outs], [o["systems"] for o in outs]
            for o in outs:
                assert (o["first_hit"] == -1).all() and np.array_equal(o["flags"], ep["flags"][:, o["t0"]:o["t0"] + o["flags"].shape[1]])
            got_status, got_sys = np.concatenate(got_status, 1), np.concatenate(got_sys, 1)
            assert np.array_equal(got_status, status), name
            el = take
            assert np.array_equal(got_sys[el][:, 0], count[el])
            some = el & (count > 0)
            assert np.array_equal(got_sys[some][:, 1], np.broadcast_to(cx[:, None], el.shape)[some])
            assert np.array_equal(got_sys[some][:, 2], np.broadcast_to(cy[:, None], el.shape)[some])
            assert (np.abs(got_sys[:, :, 3:17] - mom)[el] <= ((count[:, :, None] + 4.0) * 2.0 ** -52 * mag)[el]).all(), name
            fit = status == 0
            a_seq, _ = sf.coefficients(sys[fit], fit_cfg["min_pivot"])
            a_got, _ = sf.coefficients(got_sys[fit], fit_cfg["min_pivot"])
            S, _, d = sf.scaled_system(sys[fit])
            rel = np.linalg.norm((a_got - a_seq) * d, axis=1) / np.linalg.norm(a_seq * d, axis=1)
            bound = 64.0 * EPS * np.linalg.cond(S)
            worst = max(worst, float((rel / bound).max()))
            assert (rel <= bound).all(), (name, (rel / bound).max())
            # the final state: the last eligible record's system, left alone where an env came in ended
            gone = ep["ended"] != 0
            assert np.array_equal(bits64(st[gone]), bits64(start_state(ep)[gone]))
            last = k - 1 - el[:, ::-1].argmax(1)
            has = el.any(1)
            assert np.array_equal(st[has, 0], count[np.arange(n), last][has]) and not np.isnan(st).any()
            assert np.array_equal(bits64(st[has, 3:17]), bits64(got_sys[np.arange(n), last][has][:, 3:17]))
    print(f"n={n} k={k}: largest coefficient difference / (64 eps cond(S)) = {worst:.3g}")


def test_the_rule_stops_walkers_early_late_and_never(sf, ss):
    """Approach walkers in both use_tke modes: every approaching env is stopped, the ones that walk away never; with the turbulence
    channel subtracted the estimate it stopped on is the source to 1e-3 cells, with a constant background within 20."""
    for kw, tol in (({}, 1e-3), (TKE_OFF, 20.0)):
        ep = walkers(100, 130, 6, 11)
        fit_cfg, stop_cfg = sf.check_source_fit(**kw), ss.check_source_stop()
        st, (out,) = drive(ss, ep, fit_cfg, stop_cfg, [0, 130])
        away = np.arange(100) % 5 == 4
        hit = out["first_hit"] >= 0
        assert hit[~away].mean() > 0.9 and not hit[away].any()
        steps = st[hit, ss.HIT_STEP]
        assert steps.min() >= 8 and steps.max() > steps.min() + 5                       # some early, some late
        err = np.sqrt(((st[hit, ss.EST:ss.EST + 2] - ep["src"][hit]) ** 2).sum(1))
        print(f"use_tke={not kw}: stopped {hit.sum()} of 100, steps {steps.min():.0f} .. {steps.max():.0f}, estimate error max {err.max():.3g}")
        assert np.median(err) <= tol
        assert (st[hit, ss.EST + 2] > 0).all() and (st[hit, ss.EST + 4] > 0).all()       # sigma and the emission at the stop
        assert (st[~hit, ss.HIT_STEP] == 0).all() and (st[~hit, ss.EST:] == 0).all()


def test_placed_hits_lanes_chunk_starts_done_records_and_idle_envs(sf, ss):
    for name, ep, kw, skw, split, at in placed_hits():
        fit_cfg, stop_cfg = sf.check_source_fit(**kw), ss.check_source_stop(**skw)
        n, k = ep["flags"].shape
        cuts = [0, k] if split is None else [0, split, k]
        st, outs = drive(ss, ep, fit_cfg, stop_cfg, cuts)
        fh = outs[-1]["first_hit"] + cuts[-2]
        if at is None:
            hit = st[:, ss.HIT_STEP] > 0
            d2 = ((ep["pos"][hit, st[hit, ss.HIT_STEP].astype(int) - 1].astype(np.float64) - st[hit, ss.EST:ss.EST + 2]) ** 2).sum(1)
            assert hit.sum() >= 5 and (d2 <= 36.0).all() and (st[hit, ss.HIT_STEP] > 12).any()       # `near` held some back
            continue
        early = (st[:, ss.HIT_STEP] == at + 1)
        assert early.sum() >= 5, name
        assert (fh[early] == at).all()
        if split is not None:
            assert (outs[0]["first_hit"] == -1).all() and (outs[-1]["first_hit"][early] == 0).all()
            assert (outs[0]["state"][early, ss.RUN] >= stop_cfg["patience"]).all()        # the run came in with the state
        if "done" in name:
            assert early[0] and outs[0]["flags"][0, 40] == 3 | 8
        # the whole chunk in one piece decides the same
        st1, (one,) = drive(ss, ep, fit_cfg, stop_cfg, [0, k])
        assert np.array_equal(one["first_hit"], np.where(st[:, ss.HIT_STEP] > 0, st[:, ss.HIT_STEP] - 1, -1))
        # envs that come in already hit, or ended: untouched to the bit, first_hit -1, no estimates
        again = ss.stop_scan_chunk(ep["flags"], ep["obs"], ep["pos"], k, st, ep["ended"], fit_cfg, stop_cfg)
        was = st[:, ss.HIT_STEP] > 0
        assert (again["first_hit"][was] == -1).all() and np.array_equal(bits64(again["state"][was]), bits64(st[was]))
        assert (again["status_steps"][was] == 255).all() and np.array_equal(again["flags"][was], ep["flags"][was])
        ended = np.ones(n, np.uint8)
        gone = ss.stop_scan_chunk(ep["flags"], ep["obs"], ep["pos"], 0, start_state(ep), ended, fit_cfg, stop_cfg)
        assert (gone["first_hit"] == -1).all() and not gone["state"].any() and (gone["status_steps"] == 255).all()


@pytest.mark.parametrize("shape", [(96, 130, 6, 0), (65, 130, 6, 1)])
def test_marked_flags_give_the_episode_end_the_rule_decided(sf, ss, shape):
    """The marked flags through eval_track.reduce_chunk and source_fit.moments_chunk: the step, bit1 and the position of the end
    are the rule's, and the estimator's moments stop at the hit."""
    from uavppo import eval_track as et
    n, k, D, seed = shape
    for name, ep, kw in case_sets(n, k, D, seed):
        fit_cfg, stop_cfg = sf.check_source_fit(**kw), ss.check_source_stop()
        for cuts in ([0, k], [0, 31, k]):
            out = ss.stop_records([(ep["flags"][:, a:b], ep["obs"][:, a:b], ep["pos"][:, a:b]) for a, b in zip(cuts[:-1], cuts[1:])],
                                  n, fit_cfg, stop_cfg)
            steps, state, pos_end = out["ep"]
            stop = out["stop_step"]
            hit = stop > 0
            assert hit.sum() > n // 4, name
            assert (steps[hit] == stop[hit]).all() and ((state[hit] & 3) == 3).all() and not (state[~hit] & 2).any()
            i = stop[hit] - 1
            f = ep["flags"][hit, i]
            want = np.where((f & 1)[:, None] != 0, ep["obs"][hit, i, :2].astype(np.float64) * 500.0, ep["pos"][hit, i].astype(np.float64))
            assert np.array_equal(pos_end[hit], want)
            # the estimator saw the records up to the stop: its count is the scan's
            assert np.array_equal(out["fit"][0][hit, 0], out["state"][hit, 0])
            assert (out["fit"][2][hit] == 0).all()
            assert np.allclose(out["fit"][1][hit, 0:2], out["state"][hit, ss.EST:ss.EST + 2], rtol=0, atol=1e-6)
            # the same episode without the rule runs on: no end is earlier than the rule's
            plain = et.reduce_chunk(ep["flags"], ep["obs"], ep["pos"], 0, *et.fresh_episodes(n))
            late = (plain[1] & 1) != 0
            assert (plain[0][hit & late] >= stop[hit & late]).all()


def test_check_source_stop_refuses_with_reasons(ss):
    nan, inf = float("nan"), float("inf")
    assert ss.check_source_stop() == dict(settle_tol=0.5, patience=3, near=inf, min_steps=0)
    assert ss.check_source_stop(2, 5, 40, 10) == dict(settle_tol=2.0, patience=5, near=40.0, min_steps=10)
    assert ss.check_source_stop(near=inf)["near"] == inf and ss.check_source_stop(settle_tol=0)["settle_tol"] == 0.0
    for kw, what in ((dict(settle_tol=-0.1), "settle_tol"), (dict(settle_tol=nan), "settle_tol"), (dict(settle_tol=inf), "settle_tol"),
                     (dict(settle_tol="1"), "settle_tol"), (dict(settle_tol=True), "settle_tol"), (dict(patience=0), "patience"),
                     (dict(patience=2.0), "patience"), (dict(patience=True), "patience"), (dict(patience=1 << 31), "patience"),
                     (dict(near=nan), "near"), (dict(near=-1.0), "near"), (dict(near="far"), "near"), (dict(min_steps=-1), "min_steps"),
                     (dict(min_steps=1.5), "min_steps"), (dict(min_steps=False), "min_steps")):
        with pytest.raises(ValueError, match=what):
            ss.check_source_stop(**kw)
    assert ss.option(None) is None and ss.option(False) is None and ss.option(True) == ss.check_source_stop()
    assert ss.option({"patience": 7})["patience"] == 7
    for bad in ({"patiance": 3}, 3, "on", {"patience": 0}):
        with pytest.raises(ValueError, match="source_stop|patience"):
            ss.option(bad)


def test_the_inputs_of_the_gpu_test_have_margins(sf, ss):
    """The condition on the inputs under which the device may differ from the statement in log's last bit and still decide alike:
    no env left out, every case set of tests/test_gpu_source_stop.py, one piece and every split it cuts."""
    seen = 0
    for shape in SHAPES + SPLIT_SHAPES:
        n, k, D, seed = shape
        for name, ep, kw in case_sets(n, k, D, seed):
            seen += margins(sf, ss, ep, kw, {}, (None,) + (SPLITS if shape in SPLIT_SHAPES else ()))
    for name, ep, kw, skw, split, at in placed_hits():
        seen += margins(sf, ss, ep, kw, skw, (split,))
    assert seen > 100000
