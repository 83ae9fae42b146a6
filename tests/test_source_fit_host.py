"""CPU: the numpy statement of the source estimator (uavppo/source_fit.py) on synthetic records of E3's formula
(tests/_source_fit_cases.py): it recovers the source, the width and the peak of exact plumes, gives each status where the case was
built for it, agrees with numpy's least squares, and keeps its bookkeeping under chunking.  The kernels are tested against this
statement in tests/test_gpu_source_fit.py."""
import numpy as np
import pytest

from _source_fit_cases import EXPECTED, KINDS, MIN_K, episodes, estimates

N, KK, D = 96, 48, 6


@pytest.fixture(scope="module")
def sf():
    from uavppo import source_fit
    return source_fit


@pytest.fixture(scope="module")
def case(sf):
    ep = episodes(N, KK, D)
    state = sf.moments_chunk(ep["flags"], ep["obs"], ep["pos"], ep["state"], ep["ended"])
    est, status = sf.solve(state)
    return ep, state, est, status


def bits64(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def _fitted_kinds():
    return [j for j, s in enumerate(EXPECTED) if s == 0]


def test_the_statement_recovers_source_width_and_peak(case):
    """Exact plumes, the turbulence channel subtracted, floor 1.0: the location within 1e-3 cells (50 x the 2.1e-5 of a simulated
    approach; measured on these cases: 1.8e-6 cells at most, so the statement alone stays 10 x inside the bound and more), sigma
    and the peak of 100 within 1e-6 relative."""
    ep, state, est, status = case
    sel = np.isin(ep["kind"], _fitted_kinds())
    assert sel.sum() >= N // 3 and (status[sel] == 0).all()
    err = np.sqrt(((est[sel, 0:2] - ep["src"][sel]) ** 2).sum(1))
    sig = np.abs(est[sel, 2] - ep["sigma"][sel]) / ep["sigma"][sel]
    peak = np.abs(est[sel, 3] - 100.0) / 100.0
    print(f"location error max {err.max():.3e} cells, sigma rel {sig.max():.3e}, peak rel {peak.max():.3e}")
    assert err.max() <= 1e-4                     # 10 x inside the bound: the statement alone
    assert err.max() <= 1e-3
    assert sig.max() <= 1e-6 and peak.max() <= 1e-6
    strength = 2.0 * np.pi * est[sel, 2] ** 2 * est[sel, 3]
    assert np.allclose(est[sel, 4], strength, rtol=1e-14, atol=0)


def test_every_status_arises_where_it_was_built(case, sf):
    ep, state, est, status = case
    assert KK >= MIN_K
    for j, want in enumerate(EXPECTED):
        got = status[ep["kind"] == j]
        if want is not None:
            assert (got == want).all(), (KINDS[j], got)
    assert set(status[ep["kind"] != 4]) == {0, 1, 2, 3}
    used, b, cell = sf.used_records(ep["flags"], ep["obs"], ep["pos"], ep["ended"])
    for j, m in ((8, 0), (9, 3), (10, 4), (11, 5)):
        assert (used[ep["kind"] == j].sum(1) == m).all() and (state[ep["kind"] == j, 0] == m).all(), KINDS[j]
    assert used[ep["kind"] == 5].sum() < (ep["kind"] == 5).sum() * KK * 0.7        # the clipped cells were left out
    assert not used[(ep["flags"] & 4) != 0].any() and not used[ep["kind"] == 4].any()
    # the first five are NaN unless fitted; all eight for a count of 0
    assert np.isnan(est[status != 0, 0:5]).all() and not np.isnan(est[status == 0]).any()
    assert np.isnan(est[ep["kind"] == 8]).all() and not np.isnan(est[ep["kind"] == 9, 5:8]).any()
    # four records are enough where min_samples says so: an exact fit of four parameters
    est4, st4 = sf.solve(state, min_samples=4)
    four = ep["kind"] == 10
    assert (st4[four] != 1).all() and (st4[ep["kind"] == 9] == 1).all()


def test_envs_that_come_in_ended_are_left_alone(case):
    ep, state, est, status = case
    gone = ep["kind"] == 4
    assert gone.any() and np.array_equal(bits64(state[gone]), bits64(ep["state"][gone]))
    assert not np.isnan(state).any()                                                  # no bit2 record was read


def test_the_largest_sample_is_the_first_of_the_largest(case, sf):
    ep, state, est, status = case
    used, b, cell = sf.used_records(ep["flags"], ep["obs"], ep["pos"], ep["ended"])
    for e in np.flatnonzero(used.any(1)):
        i = np.flatnonzero(used[e])
        first = i[np.argmax(b[e, i])]
        assert state[e, 17] == b[e, first] and state[e, 18] == cell[e, first, 0] and state[e, 19] == cell[e, first, 1]
        assert state[e, 1] == cell[e, i[0], 0] and state[e, 2] == cell[e, i[0], 1]   # the centre: the first used record


def test_solve_agrees_with_lstsq_on_the_weighted_system(case, sf):
    """The scaled coefficients u = a d against numpy's SVD least squares on the column-scaled weighted design, norm-wise within
    64 eps cond(scaled A)."""
    ep, state, est, status = case
    used, b, cell = sf.used_records(ep["flags"], ep["obs"], ep["pos"], ep["ended"])
    a, bad = sf.coefficients(state)
    S, h, d = sf.scaled_system(state)
    eps, worst = np.finfo(np.float64).eps, 0.0
    checked = 0
    for e in np.flatnonzero((status == 0) | (status == 3)):
        i = np.flatnonzero(used[e])
        p = (cell[e, i, 0] - state[e, 1]) / 32.0
        q = (cell[e, i, 1] - state[e, 2]) / 32.0
        X = np.stack([np.ones_like(p), p, q, p * p + q * q], 1) * b[e, i, None] / d[e][None, :]
        u_ls = np.linalg.lstsq(X, b[e, i] * np.log(b[e, i]), rcond=None)[0]
        bound = 64.0 * eps * np.linalg.cond(S[e])
        rel = np.linalg.norm(a[e] * d[e] - u_ls) / np.linalg.norm(u_ls)
        worst = max(worst, rel / bound)
        assert rel <= bound, (e, rel, bound)
        checked += 1
    print(f"largest |u - u_lstsq| / |u_lstsq| as a fraction of 64 eps cond: {worst:.3f} over {checked} envs")
    assert checked >= N // 3


@pytest.mark.parametrize("split", [1, 31, 40, 47])
def test_chunked_calls_keep_the_bookkeeping_and_the_estimate(case, sf, split):
    """Two chunks against one: the count, the centre and the largest sample are the same bits; A and g are sums in another order
    (each chunk through its own lanes and tree), equal within (records + 8) eps of the sum of the terms' magnitudes; the estimate
    stays inside the bound."""
    from uavppo import eval_track as et
    ep, whole, est, status = case
    f, o, p = ep["flags"], ep["obs"], ep["pos"]
    # ended before the second chunk: what uav_greedy_reduce made of the first (and the envs that came in ended)
    eps0 = (np.zeros(N, np.int32), ep["ended"].copy(), np.zeros((N, 2)))
    st = sf.moments_chunk(f[:, :split], o[:, :split], p[:, :split], ep["state"], eps0[1])
    mid = et.reduce_chunk(f[:, :split], o[:, :split], p[:, :split], 0, *eps0)
    st = sf.moments_chunk(f[:, split:], o[:, split:], p[:, split:], st, mid[1])
    for j in (0, 1, 2, 17, 18, 19):
        assert np.array_equal(bits64(st[:, j]), bits64(whole[:, j])), j
    used, b, cell = sf.used_records(f, o, p, ep["ended"])
    pp = (cell[:, :, 0] - whole[:, 1:2]) / 32.0
    qq = (cell[:, :, 1] - whole[:, 2:3]) / 32.0
    w = np.where(used, b * b, 0.0)
    mag = (w * np.maximum(1.0, (pp * pp + qq * qq)) ** 2 * np.maximum(1.0, np.abs(np.log(np.where(used, b, 1.0))))).sum(1)
    tol = (KK + 8) * np.finfo(np.float64).eps * mag
    assert (np.abs(st[:, 3:17] - whole[:, 3:17]) <= tol[:, None]).all()
    est2, status2 = sf.solve(st)
    sel = np.isin(ep["kind"], _fitted_kinds())
    assert np.array_equal(status2[ep["kind"] != 4], status[ep["kind"] != 4])
    assert np.sqrt(((est2[sel, 0:2] - ep["src"][sel]) ** 2).sum(1)).max() <= 1e-3
    # the statement's own driver takes the same path
    st3, est3, status3 = sf.fit_records([(f[:, :split], o[:, :split], p[:, :split]), (f[:, split:], o[:, split:], p[:, split:])], N)
    live = ep["kind"] != 4
    assert np.array_equal(bits64(st3[live]), bits64(st[live]))


def test_the_constant_background_route(sf):
    """Without the turbulence channel b = 100 obs[2] - background: exact where the background is the true constant."""
    ep = episodes(N, KK, D, seed=3)
    obs = ep["obs"].copy()
    tke = obs[:, :, 3].astype(np.float64) * 9.0
    obs[:, :, 2] = np.where(obs[:, :, 2] < 1.0, ((obs[:, :, 2].astype(np.float64) * 100.0 - tke + 2.9) / 100.0), 1.0).astype(np.float32)
    obs[:, :, 3] = np.nan                                                             # never read on this route
    state = sf.moments_chunk(ep["flags"], obs, ep["pos"], ep["state"], ep["ended"], use_tke=False, background=2.9)
    est, status = sf.solve(state)
    sel = np.isin(ep["kind"], (0, 2, 3))
    assert (status[sel] == 0).all() and not np.isnan(state).any()
    assert np.sqrt(((est[sel, 0:2] - ep["src"][sel]) ** 2).sum(1)).max() <= 1e-3


def test_summarise_counts_what_it_is_given(sf):
    est, status, src = estimates(300)
    out = sf.summarise(est, status, src, 500.0 / 16.0, 100.0, 5.0)
    S = out["sums"]
    fit = status == 0
    err = np.sqrt(((est[:, 0:2] - src) ** 2).sum(1))
    assert S[0] == 300 and S[1] == fit.sum() and S[2] == (status == 1).sum() and S[3] == (status == 2).sum() and S[4] == (status == 3).sum()
    assert S[1] + S[2] + S[3] + S[4] == 300
    assert np.isclose(S[5], err[fit].sum(), rtol=1e-13) and np.isclose(S[6], (err[fit] ** 2).sum(), rtol=1e-13)
    assert out["loc_err"][5] == 5.0 and S[7] == (err[fit] <= 5.0).sum()
    assert np.isnan(out["loc_err"][~fit]).all()
    has = ~np.isnan(est[:, 7])
    assert S[11] == has.sum() and 0 < has.sum() < 300
    assert np.isclose(S[10], np.sqrt(((est[has, 5:7] - src[has]) ** 2).sum(1)).sum(), rtol=1e-13)
    unknown = sf.summarise(est, status, src, float("nan"), float("inf"), 5.0)["sums"]
    assert unknown[8] == 0.0 and unknown[9] == 0.0 and S[8] > 0.0 and S[9] > 0.0
    assert np.array_equal(bits64(unknown[:8]), bits64(S[:8]))
    bad = src.copy()
    bad[5, 0] = np.nan
    nan = sf.summarise(est, status, bad, 30.0, 100.0, 5.0)
    assert np.isnan(nan["sums"][5]) and np.isnan(nan["loc_err"][5]) and nan["sums"][7] == S[7] - 1
    row = sf.source_row(S)
    assert len(row) == len(sf.SOURCE_COLUMNS) and row[0] == S[1] / 300 and np.isclose(row[1], S[5] / S[1])


def test_check_source_fit_refuses_with_the_reason(sf):
    ok = sf.check_source_fit()
    assert ok == dict(use_tke=True, min_samples=5, background=0.0, floor=1.0, min_pivot=1e-6, loc_tol=5.0)
    for kw, what in ((dict(use_tke=1), "use_tke"), (dict(min_samples=3), "min_samples"), (dict(min_samples=5.0), "min_samples"),
                     (dict(min_samples=True), "min_samples"), (dict(background=float("nan")), "background"),
                     (dict(background="2.9"), "background"), (dict(floor=float("inf")), "floor"), (dict(floor=-1.0), "floor"),
                     (dict(min_pivot=0.0), "min_pivot"), (dict(min_pivot=float("nan")), "min_pivot"),
                     (dict(loc_tol=float("nan")), "loc_tol"), (dict(loc_tol=-1.0), "loc_tol")):
        with pytest.raises(ValueError, match=what):
            sf.check_source_fit(**kw)
    assert sf.option(None) is None and sf.option(False) is None and sf.option(True) == ok
    assert sf.option({"floor": 20.0, "use_tke": False, "background": 2.9})["floor"] == 20.0
    with pytest.raises(ValueError, match="flor"):
        sf.option({"flor": 2.0})
    with pytest.raises(ValueError, match="source_fit"):
        sf.option("yes")
    assert sf.variant_truth("v2.0") == (31.25, 100.0) and sf.variant_truth("v2.1") == (15.0, 100.0)
