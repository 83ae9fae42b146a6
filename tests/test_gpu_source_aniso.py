"""csrc/source_aniso.hip against the numpy statement of uavppo/source_aniso.py: uav_plume_bank (its turbulence against
uav_env_materialise bit for bit and against oracle/procedural_oracle.py, its plume against plume_base), uav_source_moments6,
uav_source_solve6, uav_source_summary6, their refusals, and the six-term model through evaluate(), EvalTracker and VecPPOTrainer on
an "aniso:8" bank."""
import ctypes as C

import numpy as np
import pytest
import torch

from _source_aniso_cases import EXPECTED, K, clean_walkers, episodes6, estimates6

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIELD_ATOL = 1e-11                                              # tests/test_gpu_procedural.py's bound for the same lines
EXACT = [0, 1, 2] + list(range(3, 24)) + [30, 31, 32]          # count, centre, A, largest sample
G = list(range(24, 30))
MIN_PIVOT = 1e-6


@pytest.fixture(scope="module")
def ops():
    from uavppo import ops as o
    return o


@pytest.fixture(scope="module")
def sa():
    from uavppo import source_aniso
    return source_aniso


@pytest.fixture(scope="module")
def sf():
    from uavppo import source_fit
    return source_fit


def bits64(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------ uav_plume_bank
SEED, SIGMA = 20261, 500.0 / 16.0


@pytest.fixture(scope="module")
def plume(ops, sa):
    """F = 3: a round field on env 0's own source, two stretched ones with theta in different quadrants, the last with its source 30
    cells from a corner (e > 300 occurs).  (params, bank as numpy, the generating env)"""
    from uavppo.vec_env import VecMethaneEnv
    env = VecMethaneEnv(3, "v2.0", DEV, seed=SEED)
    env.reset()
    src0 = env.peek()[1][0].cpu().numpy()
    params = sa.plume_params([src0, [260.5, 181.25], [30.0, 470.0]], [SIGMA, 41.0, 24.0], [SIGMA, 16.0, 8.0], [0.0, 0.6, 2.2],
                             [100.0, 100.0, 80.0])
    bank = ops.plume_bank(params, SEED, 0, device=DEV)
    torch.cuda.synchronize()
    return params, bank.cpu().numpy(), env, bank


def test_plume_bank_turbulence_is_the_procedural_field_s(ops, plume):
    """tke bit-equal to uav_env_materialise's for the same seed and global index at episode 0, within FIELD_ATOL of the oracle's;
    the round field's conc within 1e-11 of uav_env_materialise's."""
    from oracle import procedural_oracle as pr
    params, bank, env, _ = plume
    assert bank.shape == (3, 500, 500, 2) and np.isfinite(bank).all()
    for f in range(3):
        mat = ops.env_materialise(env.state, 3, env.cfg(), f).cpu().numpy()
        assert np.array_equal(bits64(bank[f, :, :, 1]), bits64(mat[:, :, 1])), f
        _, _, tke = pr.full_field(SEED, f, 0, SIGMA)
        assert np.abs(bank[f, :, :, 1] - tke).max() <= FIELD_ATOL, f
        if f == 0:
            assert np.abs(bank[0, :, :, 0] - mat[:, :, 0]).max() <= 1e-11


def test_plume_bank_concentration_is_the_statement_s(sa, plume):
    params, bank, _, _ = plume
    x, y = np.meshgrid(np.arange(500.0), np.arange(500.0), indexing="ij")
    for f in range(3):
        base = sa.plume_base(params[f], x, y)
        want = np.clip(base + bank[f, :, :, 1], 0.0, 100.0)
        assert np.abs(bank[f, :, :, 0] - want).max() <= 1e-11, f
        assert bank[f, :, :, 0].min() >= 0.0 and bank[f, :, :, 0].max() <= 100.0
    assert (sa.plume_base(params[2], x, y) == 0.0).any()                     # e > 300 occurred
    far = sa.plume_base(params[2], x, y) == 0.0
    assert np.array_equal(bits64(bank[2, :, :, 0][far]), bits64(np.clip(bank[2, :, :, 1][far], 0.0, 100.0)))
    # stretched: along the major axis the plume reaches further than across it
    cs, sn = params[1, 4], params[1, 5]
    along = sa.plume_base(params[1], 260.5 + 40.0 * cs, 181.25 + 40.0 * sn)
    across = sa.plume_base(params[1], 260.5 - 40.0 * sn, 181.25 + 40.0 * cs)
    assert along > 10.0 * across


def test_an_env_stepped_through_the_bank_sees_its_cells(plume):
    from uavppo.vec_env import VecMethaneEnv
    params, bank, _, bank_dev = plume
    n = 6
    env = VecMethaneEnv(n, "v2.0", DEV, seed=5, bank=bank_dev, bank_sources=dev(params[:, 0:2].copy()))
    env.current_radius = 1.0
    obs = env.reset().cpu().numpy()
    f = np.arange(n) % 3
    assert np.array_equal(env.peek()[1].cpu().numpy(), params[f, 0:2])
    assert np.array_equal(obs[:, 2], (bank[f, 0, 0, 0] / 100.0).astype(np.float32))
    for t in range(6):
        act = torch.full((n,), 1 + (t % 2) * 2, dtype=torch.int32, device=DEV)       # up, right, up, ...
        obs, _, done, _ = env.step(act)
        assert not bool((done > 0.5).any())
        pos = env.peek()[0].cpu().numpy()
        cx, cy = np.clip(pos[:, 0].astype(np.int32), 0, 499), np.clip(pos[:, 1].astype(np.int32), 0, 499)
        o = obs.cpu().numpy()
        assert np.array_equal(o[:, 2], (bank[f, cx, cy, 0] / 100.0).astype(np.float32)), t
        assert np.array_equal(o[:, 3], (bank[f, cx, cy, 1] / 9.0).astype(np.float32)), t


def test_synthesise_aniso_and_the_bank_specs(sa):
    from uavppo import field_bank as fb
    bank, src, truth = fb.load_with_truth("aniso:2:2-2.5", device=DEV)
    assert bank.shape == (2, 500, 500, 2) and src.shape == (2, 2) and truth.shape == (2, 4) and truth.dtype == torch.float64
    t, s = truth.cpu().numpy(), src.cpu().numpy()
    assert ((s >= 50.0) & (s <= 450.0)).all() and ((t[:, 0] / t[:, 1] >= 2.0) & (t[:, 0] / t[:, 1] <= 2.5)).all()
    assert ((t[:, 0] >= 20.0) & (t[:, 0] <= 45.0)).all() and ((t[:, 2] >= 0.0) & (t[:, 2] < np.pi)).all() and (t[:, 3] == 100.0).all()
    b2, s2 = fb.load("aniso:2:2-2.5", device=DEV)
    assert torch.equal(b2, bank) and torch.equal(s2, src)                      # seeded: the same bank again
    x, y = np.meshgrid(np.arange(500.0), np.arange(500.0), indexing="ij")
    b = bank.cpu().numpy()
    want = np.clip(sa.plume_base(sa.plume_params(s, t[:, 0], t[:, 1], t[:, 2], t[:, 3])[1], x, y) + b[1, :, :, 1], 0.0, 100.0)
    assert np.abs(b[1, :, :, 0] - want).max() <= 1e-11


# ------------------------------------------------------------------------------------------ uav_source_moments6
def _moments6(ops, chunks, start, **kw):
    st = dev(start.copy())
    cfg = ops.source_fit_cfg(**{"min_samples": 8, **kw})
    for flags, obs, pos, ended in chunks:
        ops.source_moments6({"flags": dev(flags), "obs": dev(obs), "pos": dev(pos)}, cfg, st, None if ended is None else dev(ended))
    return st.cpu().numpy()


def _g_bound6(sf, flags, obs, pos, ended, state, **kw):
    """tests/test_gpu_source_fit.py's allowance for the four-term g, with the six basis functions: (n_used + 4) 2^-52 sum |w phi_j
    ln b| per env and j, from the statement's own records and the final centre"""
    used, b, cell = sf.used_records(flags, obs, pos, ended, **kw)
    p = (cell[:, :, 0] - state[:, 1:2]) / 32.0
    q = (cell[:, :, 1] - state[:, 2:3]) / 32.0
    bu = np.where(used, b, 1.0)
    t = np.where(used, bu * bu * np.abs(np.log(bu)), 0.0)
    phi = np.stack([np.ones_like(p), np.abs(p), np.abs(q), p * p, np.abs(p * q), q * q], 2)
    return (used.sum(1) + 4.0)[:, None] * 2.0 ** -52 * (t[:, :, None] * phi).sum(1)


def _same6(got, want, bound):
    assert np.array_equal(bits64(got[:, EXACT]), bits64(want[:, EXACT]))
    assert (np.abs(got[:, G] - want[:, G]) <= bound).all()
    assert not np.isnan(got).any()                                       # no bit2 record was read


@pytest.mark.parametrize("D", [6, 8])
@pytest.mark.parametrize("k", [1, 63, 64, 65, 130])
def test_source_moments6_is_moments_chunk6(ops, sa, sf, k, D):
    """n = 24: every kind of episodes6() twice.  With `ended` (sentinels untouched to the bit) and without, in one chunk and in two
    with uav_greedy_reduce's state between them."""
    from uavppo import eval_track as et
    n = 24
    ep = episodes6(n, k, D)
    f, o, p = ep["flags"], ep["obs"], ep["pos"]
    assert np.isnan(o[(f & 4) != 0]).all()
    want = sa.moments_chunk6(f, o, p, ep["state"], ep["ended"])
    got = _moments6(ops, [(f, o, p, ep["ended"])], ep["state"])
    _same6(got, want, _g_bound6(sf, f, o, p, ep["ended"], want))
    gone = ep["ended"] != 0
    assert np.array_equal(bits64(got[gone]), bits64(ep["state"][gone]))   # untouched to the bit
    start = np.zeros_like(ep["state"])
    want0 = sa.moments_chunk6(f, o, p, start, None)
    _same6(_moments6(ops, [(f, o, p, None)], start), want0, _g_bound6(sf, f, o, p, None, want0))
    if k >= 63:
        assert (want[:, 0] >= 8).sum() >= n // 2
        for s in (31, 64 if k > 64 else 40):
            e0 = (np.zeros(n, np.int32), ep["ended"].copy(), np.zeros((n, 2)))
            mid = et.reduce_chunk(f[:, :s], o[:, :s], p[:, :s], 0, *e0)
            w1 = sa.moments_chunk6(f[:, :s], o[:, :s], p[:, :s], ep["state"], e0[1])
            want2 = sa.moments_chunk6(f[:, s:], o[:, s:], p[:, s:], w1, mid[1])
            got2 = _moments6(ops, [(f[:, :s], o[:, :s], p[:, :s], e0[1]), (f[:, s:], o[:, s:], p[:, s:], mid[1])], ep["state"])
            bound = _g_bound6(sf, f[:, :s], o[:, :s], p[:, :s], e0[1], want2) + _g_bound6(sf, f[:, s:], o[:, s:], p[:, s:], mid[1], want2)
            _same6(got2, want2, bound)


def test_source_moments6_without_the_turbulence_channel(ops, sa, sf):
    ep = episodes6(24, 65, 6, seed=2)
    kw = dict(use_tke=False, background=2.9, floor=20.0)
    obs = ep["obs"].copy()
    obs[:, :, 3] = np.nan                                                # not read on this route
    start = np.zeros_like(ep["state"])
    want = sa.moments_chunk6(ep["flags"], obs, ep["pos"], start, None, **kw)
    got = _moments6(ops, [(ep["flags"], obs, ep["pos"], None)], start, **kw)
    _same6(got, want, _g_bound6(sf, ep["flags"], obs, ep["pos"], None, want, **kw))
    assert (want[:, 0] > 0).sum() > 12


# ------------------------------------------------------------------------------------------ uav_source_solve6
def _solve6(ops, state, **kw):
    n = state.shape[0]
    est = torch.full((n, ops.SRC6_EST_N), -7.0, dtype=torch.float64, device=DEV)
    status = torch.full((n,), 99, dtype=torch.uint8, device=DEV)
    ops.source_solve6(dev(state), ops.source_fit_cfg(**{"min_samples": 8, **kw}), est, status)
    return est.cpu().numpy(), status.cpu().numpy()


def _pivots_are_clear(sa, state, min_samples, min_pivot):
    """No env that reaches the pivot test has its smallest pivot within a factor 100 of min_pivot (a pivot that is not finite is
    DEGENERATE on either side: it comes from an exact 0 / 0)."""
    _, _, low = sa.coefficients6(state, min_pivot)
    tested = (state[:, 0] >= min_samples) & np.isfinite(low)
    return not ((low[tested] > min_pivot / 100.0) & (low[tested] < min_pivot * 100.0)).any()


def _check_solve6(est, status, want_est, want_status, truth):
    assert np.array_equal(status, want_status)                           # every env: none is left out
    fit = want_status == 0
    assert np.isnan(est[~fit, 0:7]).all()
    assert np.array_equal(bits64(est[:, 7:10]), bits64(want_est[:, 7:10]))
    assert (np.abs(est[fit, 0:2] - want_est[fit, 0:2]) <= 1e-6).all()
    for j in (2, 3, 5, 6):
        assert (np.abs(est[fit, j] - want_est[fit, j]) <= 1e-9 * np.abs(want_est[fit, j])).all(), j
    angled = fit & (truth[:, 0] / truth[:, 1] >= 1.2)
    assert (np.abs(est[angled, 4] - want_est[angled, 4]) <= 1e-9).all()
    return int(fit.sum()), int(angled.sum())


@pytest.mark.parametrize("n,k", [(24, 63), (48, 64), (257, 130)])
def test_source_solve6_is_solve6_on_every_kind(ops, sa, n, k):
    ep = episodes6(n, k, 6)
    state = sa.moments_chunk6(ep["flags"], ep["obs"], ep["pos"], ep["state"], ep["ended"])
    for kw in (dict(min_samples=8, min_pivot=MIN_PIVOT), dict(min_samples=6, min_pivot=1e-12)):
        assert _pivots_are_clear(sa, state, kw["min_samples"], kw["min_pivot"])
        want_est, want_status = sa.solve6(state, **kw)
        est, status = _solve6(ops, state, **kw)
        _check_solve6(est, status, want_est, want_status, ep["truth"])
    live = ep["ended"] == 0
    assert set(want_status[live]) == {0, 1, 2, 3}
    want_est, want_status = sa.solve6(state)
    for e in np.where(live)[0]:
        assert want_status[e] == EXPECTED[e % K], (e, want_status[e])


def test_source_solve6_recovers_the_clean_walkers(ops, sa):
    """The device's answer on the recipe of tests/test_source_aniso_host.py: every env fitted, the statement's values."""
    ep = clean_walkers(n=130)
    state = _moments6(ops, [(ep["flags"], ep["obs"], ep["pos"], None)], np.zeros((130, 33)))
    assert _pivots_are_clear(sa, state, 8, MIN_PIVOT)
    want_est, want_status = sa.solve6(state)
    est, status = _solve6(ops, state)
    fitted, angled = _check_solve6(est, status, want_est, want_status, ep["truth"])
    assert fitted == 130 and angled == 130
    assert np.hypot(est[:, 0] - ep["src"][:, 0], est[:, 1] - ep["src"][:, 1]).max() <= 1e-5
    assert (np.abs(est[:, 2:4] - ep["truth"][:, 0:2]) <= 1e-6 * ep["truth"][:, 0:2]).all()


# ------------------------------------------------------------------------------------------ uav_source_summary6
def _summary6(ops, est, status, src, truth, loc_tol, per_env=True):
    n = status.shape[0]
    sums = torch.full((ops.SRC6_SUM_N,), -7.0, dtype=torch.float64, device=DEV)
    loc = torch.full((n,), -7.0, dtype=torch.float64, device=DEV) if per_env else None
    ops.source_summary6(dev(est), dev(status), dev(src), None if truth is None else dev(truth), loc_tol, sums, loc_err=loc)
    return sums.cpu().numpy(), None if loc is None else loc.cpu().numpy()


@pytest.mark.parametrize("n", [1, 255, 256, 257, 600])
def test_source_summary6_is_summarise6(ops, sa, n):
    est, status, src, truth = estimates6(n)
    if n > 7:
        assert np.isnan(truth).any(1).sum() > 0 and np.isfinite(truth).all(1).sum() > 0
    for tr in (truth, None):
        want = sa.summarise6(est, status, src, tr, 5.0)
        sums, loc = _summary6(ops, est, status, src, tr, 5.0)
        assert np.array_equal(bits64(sums), bits64(want["sums"])), (sums, want["sums"])
        assert np.array_equal(bits64(loc), bits64(want["loc_err"]))
        sums2, _ = _summary6(ops, est, status, src, tr, 5.0, per_env=False)      # the per-env output is optional
        assert np.array_equal(bits64(sums2), bits64(sums))
    if n > 7:
        assert want["loc_err"][5] == 5.0


def test_source_fit_aniso_class_runs_the_three(ops, sa, sf):
    """SourceFit(model="aniso"): restart / chunk / finish over two chunks equals the statement's driver."""
    from uavppo import eval_track as et
    n, k = 48, 80
    ep = episodes6(n, k, 6, seed=4)
    ep["ended"][:] = 0
    fit = sf.SourceFit(n, DEV, model="aniso")
    fit.state.fill_(3.0)
    fit.restart()
    state = [dev(a) for a in et.fresh_episodes(n)]
    for t0 in (0, 50):
        recs = {key: dev(ep[key][:, t0:t0 + 50]) for key in ("flags", "obs", "pos")}
        fit.chunk(recs, state[1])
        ops.greedy_reduce(recs, t0, *state)
    sums = fit.finish(dev(ep["src"]), truth=dev(ep["truth"])).cpu().numpy()
    chunks = [(ep["flags"][:, :50], ep["obs"][:, :50], ep["pos"][:, :50]), (ep["flags"][:, 50:], ep["obs"][:, 50:], ep["pos"][:, 50:])]
    st, est, status = sa.fit_records6(chunks, n)
    assert np.array_equal(bits64(fit.state.cpu().numpy()[:, EXACT]), bits64(st[:, EXACT]))
    assert _pivots_are_clear(sa, st, 8, MIN_PIVOT)
    m = fit.metrics()
    assert np.array_equal(m["source_status"], status)
    ok = status == 0
    assert np.abs(m["source_estimate"][ok] - est[ok, 0:2]).max() <= 1e-6
    assert np.allclose(m["source_sigma_minor"][ok], est[ok, 3], rtol=1e-9, atol=0) and np.allclose(m["source_theta"][ok], est[ok, 4], rtol=0, atol=1e-9)
    assert sums[0] == n and sums[1] == ok.sum() and sums[15] == ok.sum()


# ------------------------------------------------------------------------------------------ refusals
def test_the_entry_points_refuse_with_a_reason(ops, sa):
    from uavppo import _lib
    lib, h = _lib.lib(), ops.Context.get(torch.device(DEV)).handle
    a = torch.full((4096,), -3.0, dtype=torch.float64, device=DEV)
    p = C.c_void_p(a.data_ptr())
    odd = C.c_void_p(a.data_ptr() + 4)
    nan, inf = float("nan"), float("inf")

    def cfg(**kw):
        return C.byref(ops.source_fit_cfg(**{"min_samples": 8, **kw}))

    g = cfg()
    for args, what in (((None, p, p, 1, 1, 6, g, None, p), b"NULL"), ((p, p, p, 1, 1, 6, g, None, None), b"NULL"),
                       ((p, p, p, 1, 1, 6, None, None, p), b"NULL cfg"), ((p, p, p, 0, 1, 6, g, None, p), b"at least 1"),
                       ((p, p, p, 1, 0, 6, g, None, p), b"at least 1"), ((p, p, p, 1, 1, 3, g, None, p), b"at least 4"),
                       ((p, p, p, 1, 1, 2, cfg(use_tke=False), None, p), b"at least 3"),
                       ((p, p, p, 1 << 12, 1 << 12, 128, g, None, p), b"2^31"),
                       ((p, p, p, 1, 1, 6, cfg(min_samples=5), None, p), b"min_samples"),
                       ((p, p, p, 1, 1, 6, cfg(floor=nan), None, p), b"floor"), ((p, p, p, 1, 1, 6, cfg(floor=inf), None, p), b"floor"),
                       ((p, p, p, 1, 1, 6, cfg(background=nan), None, p), b"background"),
                       ((p, p, p, 1, 1, 6, cfg(min_pivot=0.0), None, p), b"min_pivot"),
                       ((p, p, p, 1, 1, 6, cfg(min_pivot=inf), None, p), b"min_pivot"),
                       ((p, p, odd, 1, 1, 6, g, None, p), b"aligned")):
        assert lib.uav_source_moments6(h, *args, None) == 2 and what in lib.uav_last_error(), (what, lib.uav_last_error())
    for args, what in (((None, 1, g, p, p), b"NULL"), ((p, 1, g, None, p), b"NULL"), ((p, 1, g, p, None), b"NULL"),
                       ((p, 1, None, p, p), b"NULL cfg"), ((p, 0, g, p, p), b"at least 1"),
                       ((p, 1, cfg(min_samples=5), p, p), b"min_samples"), ((p, 1, cfg(min_pivot=-1.0), p, p), b"min_pivot")):
        assert lib.uav_source_solve6(h, *args, None) == 2 and what in lib.uav_last_error(), what
    for args, what in (((None, p, p, None, 1, 5.0, None, p), b"NULL"), ((p, None, p, None, 1, 5.0, None, p), b"NULL"),
                       ((p, p, None, None, 1, 5.0, None, p), b"NULL"), ((p, p, p, None, 1, 5.0, None, None), b"NULL"),
                       ((p, p, p, None, 0, 5.0, None, p), b"at least 1"), ((p, p, p, p, 1, nan, None, p), b"NaN")):
        assert lib.uav_source_summary6(h, *args, None) == 2 and what in lib.uav_last_error(), what
    good = sa.plume_params([[100.0, 200.0]], 30.0, 12.0, 0.7, 90.0)

    def row(j=None, v=None):
        r = good.copy()
        if j is not None:
            r[0, j] = v
        return r

    def hp(r):
        return r.ctypes.data_as(C.c_void_p)

    rows = [(row(0, nan), b"not finite"), (row(7, inf), b"not finite"), (row(2, 0.0), b"widths"), (row(3, -2.0), b"widths"),
            (row(6, 0.0), b"peak"), (row(4, 0.9), b"cos^2")]
    for r, what in rows:
        assert lib.uav_plume_bank(h, hp(r), 1, 7, 0, p, None) == 2 and what in lib.uav_last_error(), what
    g1 = row()
    for args, what in (((None, 1, 7, 0, p), b"NULL"), ((hp(g1), 1, 7, 0, None), b"NULL"), ((hp(g1), 0, 7, 0, p), b"at least 1"),
                       ((hp(g1), 1, 7, -1, p), b"index0"), ((hp(g1), 1, 7, 0, C.c_void_p(a.data_ptr() + 8)), b"aligned")):
        assert lib.uav_plume_bank(h, *args, None) == 2 and what in lib.uav_last_error(), what
    torch.cuda.synchronize()
    assert bool((a == -3.0).all())                                       # nothing was launched: every buffer stands


# ------------------------------------------------------------------------------------------ end to end
N, STEPS, CHUNK = 64, 120, 50


@pytest.fixture(scope="module")
def aniso8():
    from uavppo import field_bank as fb
    return fb.load_with_truth("aniso:8", device=DEV)


def make_env(b, n=N, seed=3):
    from uavppo.vec_env import VecMethaneEnv
    env = VecMethaneEnv(n, "v2.0", DEV, seed=seed, bank=b[0], bank_sources=b[1])
    env.current_radius = 2.0
    return env


def make_policy(kind):
    from uavppo.policy import LSTMActorCritic, MLPActorCritic
    return LSTMActorCritic(6, 64, 1, device=DEV, seed=3) if kind == "lstm" else MLPActorCritic(6, 5, device=DEV, seed=1)


def greedy_records(policy, env):
    """The records evaluate() reads, chunk by chunk, as numpy (as tests/test_gpu_source_fit_eval.py takes them)"""
    from uavppo.greedy import GreedyRun, policy_core
    kind, core = policy_core(policy)
    env.reset()
    run = GreedyRun(kind, core, env)
    out = []
    for t0 in range(0, STEPS, CHUNK):
        recs = run.chunk(t0, min(CHUNK, STEPS - t0))
        out.append(tuple(recs[k].cpu().numpy().copy() for k in ("flags", "obs", "pos")))
    return out


def _sure(sa, st):
    """Envs whose status does not hang on a last bit: the smallest pivot clear of min_pivot, det and trace clear of 0"""
    a, _, low = sa.coefficients6(st)
    with np.errstate(all="ignore"):
        l11, l12, l22 = -2.0 * a[:, 3], -a[:, 4], -2.0 * a[:, 5]
        det, trace = l11 * l22 - l12 * l12, l11 + l22
        scale = l11 * l11 + l22 * l22 + l12 * l12
        edge = (np.abs(det) <= 1e-9 * scale) | (np.abs(trace) <= 1e-9 * np.sqrt(scale))
        near = np.isfinite(low) & (low > MIN_PIVOT / 100.0) & (low < MIN_PIVOT * 100.0)
    return ~((st[:, 0] >= 8) & (near | (np.isfinite(low) & (low >= MIN_PIVOT) & edge)))


@pytest.mark.parametrize("kind", ["lstm", "mlp"])
def test_evaluate_aniso_is_the_statement_on_its_records(aniso8, sa, kind):
    from evaluate_with_lstm import evaluate
    pol = make_policy(kind)
    plain = evaluate(pol, make_env(aniso8), max_steps=STEPS, chunk=CHUNK)
    m = evaluate(pol, make_env(aniso8), max_steps=STEPS, chunk=CHUNK, source_fit={"model": "aniso"}, bank_truth=aniso8[2])
    for key in plain:                                           # steps, successes, deviations: exactly those without the option
        assert np.array_equal(plain[key], m[key]) and plain[key].dtype == m[key].dtype, key
    assert sorted(set(m) - set(plain)) == ["source_error", "source_estimate", "source_max_sample", "source_peak", "source_sigma",
                                           "source_sigma_minor", "source_status", "source_strength", "source_theta"]
    env = make_env(aniso8)
    chunks = greedy_records(pol, env)
    src = env.peek()[1].cpu().numpy().astype(np.float64)
    st, est, status = sa.fit_records6(chunks, N)
    sure = _sure(sa, st)
    fit = sure & (status == 0)
    print(f"\n[{kind}] fitted {int((status == 0).sum())} / {N}; statuses {np.bincount(status, minlength=4).tolist()}; sure {int(sure.sum())}")
    assert np.array_equal(m["source_status"][sure], status[sure]) and m["source_status"].dtype == np.uint8
    assert np.array_equal(bits64(m["source_max_sample"][sure]), bits64(est[sure, 7:10]))
    if fit.any():
        assert np.abs(m["source_estimate"][fit] - est[fit, 0:2]).max() <= 1e-6
        for key, j in (("source_sigma", 2), ("source_sigma_minor", 3), ("source_peak", 5), ("source_strength", 6)):
            assert np.allclose(m[key][fit], est[fit, j], rtol=1e-9, atol=0), key
        err = np.hypot(est[:, 0] - src[:, 0], est[:, 1] - src[:, 1])
        assert np.abs(m["source_error"][fit] - err[fit]).max() <= 2e-6
    assert np.isnan(m["source_error"][sure & (status != 0)]).all()
    # the truth rows came by the field rule: env e's episode 0 reads field e mod 8
    assert np.array_equal(src, aniso8[1].cpu().numpy()[np.arange(N) % 8])


def test_evaluate_refuses_what_the_six_term_model_does_not_cover(aniso8):
    from evaluate_with_lstm import evaluate
    pol, env = make_policy("lstm"), make_env(aniso8)
    with pytest.raises(ValueError, match="four-term"):
        evaluate(pol, env, max_steps=8, source_fit={"model": "aniso"}, source_stop=True)
    with pytest.raises(ValueError, match="bank_truth"):
        evaluate(pol, env, max_steps=8, source_fit=True, bank_truth=aniso8[2])
    with pytest.raises(ValueError, match="bank_truth"):
        evaluate(pol, env, max_steps=8, source_fit={"model": "aniso"}, bank_truth=aniso8[2][:5])
    with pytest.raises(ValueError, match="min_samples"):
        evaluate(pol, env, max_steps=8, source_fit={"model": "aniso", "min_samples": 5})
    with pytest.raises(ValueError, match="controller"):
        evaluate(pol, env, max_steps=8, controller=object(), source_fit={"model": "aniso"})


def make_trainer(b, **kw):
    from uavppo.trainer import VecPPOTrainer
    return VecPPOTrainer(32, 16, device=DEV, seed=11, variant="v2.0", bank=b[0], bank_sources=b[1], policy="lstm", hidden=64, **kw)


def test_trainer_and_tracker_carry_the_sixteen_sums(aniso8, sa, sf):
    """Three iterations on the bank: parameters byte-identical with and without eval_source_fit; one EvalTracker.run() row carries
    the sums a standalone SourceFit(model="aniso") gives on the same evaluation, truth gathered by the field rule; run() reads nothing."""
    from uavppo import eval_track as et, ops
    ev = dict(eval_every=1, eval_envs=N, eval_max_steps=STEPS, eval_chunk=CHUNK, eval_radius=2.0)
    on = make_trainer(aniso8, eval_source_fit={"model": "aniso"}, bank_truth=aniso8[2], **ev)
    off = make_trainer(aniso8, **ev)
    for _ in range(3):
        on.train_iteration()
        off.train_iteration()
    same = lambda x, y: torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert same(on.policy.flat, off.policy.flat) and same(on.exp_avg, off.exp_avg) and same(on.exp_avg_sq, off.exp_avg_sq)
    assert same(on.eval_tracker.best_flat(), off.eval_tracker.best_flat())
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        on.eval_tracker.run(4)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    rows, rows_off = on.eval_tracker.curve(wait=True), off.eval_tracker.curve(wait=True)
    assert [r["iteration"] for r in rows] == [1, 2, 3, 4] and all("source" not in r for r in rows_off)
    for r, q in zip(rows, rows_off):
        assert np.array_equal(bits64(r["sums"]), bits64(q["sums"])) and np.array_equal(bits64(r["state"]), bits64(q["state"]))
        assert r["source"].shape == (16,) and r["source"][0] == N and r["source"][1:5].sum() == N
        assert r["source"][15] == r["source"][1]                            # every fitted env has its truth row
    print(f"\nfitted {[int(r['source'][1]) for r in rows]} of {N}")
    # a standalone six-term SourceFit over evaluation 4: the tracker's env arguments, the parameters as they stand
    from uavppo.greedy import GreedyRun, policy_core
    from uavppo.vec_env import VecMethaneEnv
    t = on.eval_tracker
    env = VecMethaneEnv(**t.env_args)
    env.current_radius = 2.0
    env.reset()
    src = env.peek()[1].to(torch.float64).contiguous()
    truth = aniso8[2][torch.arange(N, device=DEV) % 8].contiguous()
    k2, core = policy_core(on.policy)
    run, fit = GreedyRun(k2, core, env), sf.SourceFit(N, DEV, model="aniso")
    state = [torch.from_numpy(a).to(DEV) for a in et.fresh_episodes(N)]
    for t0 in range(0, STEPS, CHUNK):
        recs = run.chunk(t0, min(CHUNK, STEPS - t0))
        fit.chunk(recs, state[1])
        ops.greedy_reduce(recs, t0, *state)
    sums = fit.finish(src, truth=truth).cpu().numpy()
    assert np.array_equal(bits64(sums), bits64(rows[3]["source"]))
    line = et.curve_row(rows[3]["iteration"], rows[3]["sums"], rows[3]["state"], rows[3]["source"])
    assert len(line) == len(et.curve_columns(True, aniso=True)) == len(et.CURVE_COLUMNS) + 9
    with pytest.raises(ValueError, match="four-term"):
        make_trainer(aniso8, eval_source_fit={"model": "aniso"}, eval_source_stop=True, **ev)


# A bank whose sources stand near the origin, where every episode starts (the "aniso:8" sources are U[50, 450]^2: a fresh policy's 120
# steps rarely cross those plumes, and the comparison above is then one of FEW against FEW).  Wide plumes, so that the first steps
# from (0, 0) and the wind's scatter of a policy that stays or leans on the boundary give six usable records in distinct cells.
NEAR_SRC = np.array([[40.0, 40.0], [44.0, 37.0]])
NEAR_TRUTH = np.array([[80.0, 40.0, 0.5, 100.0], [70.0, 35.0, 2.4, 90.0]])


@pytest.fixture(scope="module")
def near(ops, sa):
    params = sa.plume_params(NEAR_SRC, NEAR_TRUTH[:, 0], NEAR_TRUTH[:, 1], NEAR_TRUTH[:, 2], NEAR_TRUTH[:, 3])
    return ops.plume_bank(params, 99, 0, device=DEV), dev(NEAR_SRC.copy()), dev(NEAR_TRUTH.copy())


@pytest.mark.parametrize("kind", ["lstm", "mlp"])
def test_evaluate_aniso_near_the_start_has_fits_to_compare(near, sa, kind, tmp_path):
    from evaluate_model import ModelEvaluator
    from evaluate_with_lstm import evaluate
    pol = make_policy(kind)
    cfg = {"model": "aniso", "min_samples": 6}
    m = evaluate(pol, make_env(near), max_steps=STEPS, chunk=CHUNK, source_fit=cfg, bank_truth=near[2])
    env = make_env(near)
    chunks = greedy_records(pol, env)
    src = env.peek()[1].cpu().numpy().astype(np.float64)
    st, est, status = sa.fit_records6(chunks, N, min_samples=6)
    a, _, low = sa.coefficients6(st)
    with np.errstate(all="ignore"):
        l11, l12, l22 = -2.0 * a[:, 3], -a[:, 4], -2.0 * a[:, 5]
        det, trace, scale = l11 * l22 - l12 * l12, l11 + l22, l11 * l11 + l22 * l22 + l12 * l12
        edge = np.isfinite(low) & (low >= MIN_PIVOT) & ((np.abs(det) <= 1e-9 * scale) | (np.abs(trace) <= 1e-9 * np.sqrt(scale)))
        near_pivot = np.isfinite(low) & (low > MIN_PIVOT / 100.0) & (low < MIN_PIVOT * 100.0)
    sure = ~((st[:, 0] >= 6) & (near_pivot | edge))
    fit = sure & (status == 0)
    print(f"\n[{kind}] near bank: fitted {int((status == 0).sum())} / {N}; statuses {np.bincount(status, minlength=4).tolist()}; "
          f"sure {int(sure.sum())}; median error {np.median(m['source_error'][fit]) if fit.any() else float('nan'):.3g} cells")
    assert fit.sum() >= 1, "precondition: the bank was built so that some episodes can be fitted"
    assert np.array_equal(m["source_status"][sure], status[sure])
    # mu, widths, peak: the solve amplifies the last bit of log by the system's conditioning, which these short tracks leave poor;
    # 1e-6 cells / 1e-9 relative are for pivots of 1e-2, so the comparison scales with 1e-2 / pivot
    amp = np.maximum(1.0, 1e-2 / low[fit])
    assert (np.abs(m["source_estimate"][fit] - est[fit, 0:2]).max(1) <= 1e-6 * amp).all()
    for key, j in (("source_sigma", 2), ("source_sigma_minor", 3), ("source_peak", 5), ("source_strength", 6)):
        assert (np.abs(m[key][fit] - est[fit, j]) <= 1e-9 * amp * np.abs(est[fit, j])).all(), key
    assert np.array_equal(bits64(m["source_max_sample"][sure]), bits64(est[sure, 7:10]))
    if kind == "lstm":                                          # ModelEvaluator: the same model, two more CSV columns
        ev = ModelEvaluator(pol, N, DEV, env=make_env(near))
        out = ev.run_evaluation(max_steps=STEPS, chunk=CHUNK, csv_path=str(tmp_path / "evaluation_results.csv"), source_fit=cfg,
                                bank_truth=near[2])
        lines = open(tmp_path / "source_estimates.csv").read().splitlines()
        head = lines[0].split(",")
        assert head[4:8] == ["Sigma", "Sigma_Minor", "Theta", "Peak"] and len(lines) == N + 1 and "source_theta" in out
        with pytest.raises(ValueError, match="bank_truth"):
            ev.run_evaluation(max_steps=8, csv_path=None, source_fit=True, bank_truth=near[2])
