"""csrc/source_fit.hip against the numpy statement of uavppo/source_fit.py: uav_source_moments (bit-equal in everything that goes
through no transcendental, g within the rounding of its sum), uav_source_solve and uav_source_summary.  Synthetic records only
(tests/_source_fit_cases.py); evaluate() and the trainer are in tests/test_gpu_source_fit_eval.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from _source_fit_cases import episodes, estimates

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EXACT = [0, 1, 2] + list(range(3, 13)) + [17, 18, 19]         # count, centre, A, largest sample
G = [13, 14, 15, 16]


@pytest.fixture(scope="module")
def ops():
    from uavppo import ops as o
    return o


@pytest.fixture(scope="module")
def sf():
    from uavppo import source_fit
    return source_fit


def bits64(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _moments(ops, chunks, start, **kw):
    """uav_source_moments over chunks = [(flags, obs, pos, ended or None)] from the start state -> numpy state"""
    st = dev(start.copy())
    cfg = ops.source_fit_cfg(**kw)
    for flags, obs, pos, ended in chunks:
        ops.source_moments({"flags": dev(flags), "obs": dev(obs), "pos": dev(pos)}, cfg, st, None if ended is None else dev(ended))
    return st.cpu().numpy()


def _g_bound(sf, flags, obs, pos, ended, state, **kw):
    """(n_used + 4) 2^-52 sum |w phi_j ln b| per env and j, from the statement's own records and the final centre"""
    used, b, cell = sf.used_records(flags, obs, pos, ended, **kw)
    p = (cell[:, :, 0] - state[:, 1:2]) / 32.0
    q = (cell[:, :, 1] - state[:, 2:3]) / 32.0
    bu = np.where(used, b, 1.0)
    t = np.where(used, bu * bu * np.abs(np.log(bu)), 0.0)
    phi = np.stack([np.ones_like(p), np.abs(p), np.abs(q), p * p + q * q], 2)
    return (used.sum(1) + 4.0)[:, None] * 2.0 ** -52 * (t[:, :, None] * phi).sum(1)


def _same(got, want, bound):
    assert np.array_equal(bits64(got[:, EXACT]), bits64(want[:, EXACT]))
    assert (np.abs(got[:, G] - want[:, G]) <= bound).all()
    assert not np.isnan(got).any()                                       # no bit2 record was read


@pytest.mark.parametrize("D", [6, 8])
@pytest.mark.parametrize("k", [1, 2, 63, 64, 65, 250])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_source_moments_is_moments_chunk(ops, sf, n, k, D):
    """Every kind of episodes(): ends by bit0, bit3 (stepped records behind it), both, nowhere; envs that come in ended (sentinels);
    clipped cells; collinear tracks; a bowl; 0, 3, 4, 5 usable records; NaN in the obs / pos of every bit2 record."""
    ep = episodes(n, k, D)
    assert np.isnan(ep["obs"][(ep["flags"] & 4) != 0]).all()
    want = sf.moments_chunk(ep["flags"], ep["obs"], ep["pos"], ep["state"], ep["ended"])
    got = _moments(ops, [(ep["flags"], ep["obs"], ep["pos"], ep["ended"])], ep["state"])
    _same(got, want, _g_bound(sf, ep["flags"], ep["obs"], ep["pos"], ep["ended"], want))
    gone = ep["ended"] != 0
    assert np.array_equal(bits64(got[gone]), bits64(ep["state"][gone]))   # untouched to the bit
    if n >= 63 and k >= 63:
        assert (want[:, 0] >= 5).sum() > n // 3


def test_source_moments_without_ended_and_without_the_turbulence_channel(ops, sf):
    ep = episodes(65, 65, 6, seed=2)
    kw = dict(use_tke=False, background=2.9, floor=20.0)
    obs = ep["obs"].copy()
    obs[:, :, 3] = np.nan                                                # not read on this route
    start = np.zeros_like(ep["state"])
    want = sf.moments_chunk(ep["flags"], obs, ep["pos"], start, None, **kw)
    got = _moments(ops, [(ep["flags"], obs, ep["pos"], None)], start, **kw)
    _same(got, want, _g_bound(sf, ep["flags"], obs, ep["pos"], None, want, **kw))
    assert (want[:, 0] > 0).sum() > 30


@pytest.mark.parametrize("n,k", [(65, 65), (257, 250)])
def test_source_moments_two_piece_splits(ops, sf, n, k):
    """The pieces of a chunk with uav_greedy_reduce's state between them, as the tracker issues them, equal the statement under
    the same split."""
    from uavppo import eval_track as et
    ep = episodes(n, k, 6, seed=1)
    f, o, p = ep["flags"], ep["obs"], ep["pos"]
    for s in (1, 31, 63, 64):
        e0 = (np.zeros(n, np.int32), ep["ended"].copy(), np.zeros((n, 2)))
        mid = et.reduce_chunk(f[:, :s], o[:, :s], p[:, :s], 0, *e0)
        w1 = sf.moments_chunk(f[:, :s], o[:, :s], p[:, :s], ep["state"], e0[1])
        want = sf.moments_chunk(f[:, s:], o[:, s:], p[:, s:], w1, mid[1])
        got = _moments(ops, [(f[:, :s], o[:, :s], p[:, :s], e0[1]), (f[:, s:], o[:, s:], p[:, s:], mid[1])], ep["state"])
        # each piece's g is within its own bound of the statement's; the second piece starts from the first's
        bound = (_g_bound(sf, f[:, :s], o[:, :s], p[:, :s], e0[1], want) + _g_bound(sf, f[:, s:], o[:, s:], p[:, s:], mid[1], want))
        _same(got, want, bound)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_source_solve_is_solve(ops, sf, n):
    """Fed the statement's state: status, mu, sigma and the largest sample bit-equal; peak and strength within 1e-15 relative
    (only exp differs)."""
    ep = episodes(n, 64, 6)
    state = sf.moments_chunk(ep["flags"], ep["obs"], ep["pos"], ep["state"], ep["ended"])
    for kw in (dict(), dict(min_samples=4, min_pivot=1e-3)):
        want_est, want_status = sf.solve(state, **kw)
        est = torch.full((n, ops.SRC_EST_N), -7.0, dtype=torch.float64, device=DEV)
        status = torch.full((n,), 99, dtype=torch.uint8, device=DEV)
        ops.source_solve(dev(state), ops.source_fit_cfg(**kw), est, status)
        est, status = est.cpu().numpy(), status.cpu().numpy()
        assert np.array_equal(status, want_status)
        assert np.array_equal(bits64(est[:, [0, 1, 2, 5, 6, 7]]), bits64(want_est[:, [0, 1, 2, 5, 6, 7]]))
        fit = want_status == 0
        assert np.isnan(est[~fit, 3:5]).all()
        assert (np.abs(est[fit, 3:5] - want_est[fit, 3:5]) <= 1e-15 * np.abs(want_est[fit, 3:5])).all()
    if n >= 63:
        assert set(want_status) == {0, 1, 2, 3}


def _summary(ops, est, status, src, sigma_true, peak_true, loc_tol, per_env=True):
    n = status.shape[0]
    sums = torch.full((ops.SRC_SUM_N,), -7.0, dtype=torch.float64, device=DEV)
    loc = torch.full((n,), -7.0, dtype=torch.float64, device=DEV) if per_env else None
    ops.source_summary(dev(est), dev(status), dev(src), sigma_true, peak_true, loc_tol, sums, loc_err=loc)
    return sums.cpu().numpy(), None if loc is None else loc.cpu().numpy()


@pytest.mark.parametrize("n", [1, 63, 255, 256, 257, 1024, 4097])
def test_source_summary_is_summarise(ops, sf, n):
    est, status, src = estimates(n)
    for sig, peak in ((500.0 / 16.0, 100.0), (float("nan"), float("inf"))):
        want = sf.summarise(est, status, src, sig, peak, 5.0)
        sums, loc = _summary(ops, est, status, src, sig, peak, 5.0)
        assert np.array_equal(bits64(sums), bits64(want["sums"])), (sums, want["sums"])
        assert np.array_equal(bits64(loc), bits64(want["loc_err"]))
        sums2, _ = _summary(ops, est, status, src, sig, peak, 5.0, per_env=False)        # the per-env output is optional
        assert np.array_equal(bits64(sums2), bits64(sums))
    if n > 7:
        assert want["loc_err"][5] == 5.0
    bad = src.copy()
    bad[0, 1] = np.nan                                                                    # a NaN source: defined, not an error
    want = sf.summarise(est, status, bad, 30.0, 100.0, 5.0)
    sums, loc = _summary(ops, est, status, bad, 30.0, 100.0, 5.0)
    # the same NaNs in the same places, every other sum bit-equal (a NaN's sign is not arithmetic: x - NaN keeps it on the host,
    # the device's subtraction negates the operand)
    isn = np.isnan(want["sums"])
    assert np.array_equal(np.isnan(sums), isn) and np.array_equal(bits64(sums[~isn]), bits64(want["sums"][~isn]))
    assert np.isnan(sums[5]) and np.isnan(sums[10]) and np.isnan(loc[0]) == np.isnan(want["loc_err"][0])


def test_source_fit_class_runs_the_three(ops, sf):
    """SourceFit: restart / chunk / finish over two chunks equals the statement's driver."""
    n, k = 65, 80
    ep = episodes(n, k, 6, seed=4)
    ep["ended"][:] = 0
    from uavppo import eval_track as et
    fit = sf.SourceFit(n, DEV, min_samples=5)
    fit.state.fill_(3.0)
    fit.restart()
    state = [dev(a) for a in et.fresh_episodes(n)]
    for t0 in (0, 50):
        recs = {key: dev(ep[key][:, t0:t0 + 50]) for key in ("flags", "obs", "pos")}
        fit.chunk(recs, state[1])
        ops.greedy_reduce(recs, t0, *state)
    sums = fit.finish(dev(ep["src"]), 31.25, 100.0).cpu().numpy()
    st, est, status = sf.fit_records([(ep["flags"][:, :50], ep["obs"][:, :50], ep["pos"][:, :50]),
                                      (ep["flags"][:, 50:], ep["obs"][:, 50:], ep["pos"][:, 50:])], n)
    assert np.array_equal(bits64(fit.state.cpu().numpy()[:, EXACT]), bits64(st[:, EXACT]))
    m = fit.metrics()
    same = np.abs(sf.coefficients(st)[0][:, 3]) > 1e-9
    assert np.array_equal(m["source_status"][same], status[same])
    ok = same & (status == 0)
    assert np.allclose(m["source_estimate"][ok], est[ok, 0:2], rtol=0, atol=1e-6)
    assert sums[0] == n and sums[1] == (m["source_status"] == 0).sum()


def test_the_entry_points_refuse_with_a_reason(ops):
    from uavppo import _lib
    lib, h = _lib.lib(), ops.Context.get(torch.device(DEV)).handle
    a = torch.zeros(4096, dtype=torch.float64, device=DEV)
    p = C.c_void_p(a.data_ptr())
    odd = C.c_void_p(a.data_ptr() + 4)
    good = ops.source_fit_cfg()
    nan, inf = float("nan"), float("inf")

    def cfg(**kw):
        return C.byref(ops.source_fit_cfg(**kw))

    g = C.byref(good)
    for args, what in (((None, p, p, 1, 1, 6, g, None, p), b"NULL"), ((p, p, p, 1, 1, 6, g, None, None), b"NULL"),
                       ((p, p, p, 1, 1, 6, None, None, p), b"NULL cfg"), ((p, p, p, 0, 1, 6, g, None, p), b"at least 1"),
                       ((p, p, p, 1, 0, 6, g, None, p), b"at least 1"), ((p, p, p, 1, 1, 3, g, None, p), b"at least 4"),
                       ((p, p, p, 1, 1, 2, cfg(use_tke=False), None, p), b"at least 3"),
                       ((p, p, p, 1 << 12, 1 << 12, 128, g, None, p), b"2^31"),
                       ((p, p, p, 1, 1, 6, cfg(min_samples=3), None, p), b"min_samples"),
                       ((p, p, p, 1, 1, 6, cfg(floor=nan), None, p), b"floor"), ((p, p, p, 1, 1, 6, cfg(floor=inf), None, p), b"floor"),
                       ((p, p, p, 1, 1, 6, cfg(background=nan), None, p), b"background"),
                       ((p, p, p, 1, 1, 6, cfg(min_pivot=0.0), None, p), b"min_pivot"),
                       ((p, p, p, 1, 1, 6, cfg(min_pivot=inf), None, p), b"min_pivot"),
                       ((p, p, odd, 1, 1, 6, g, None, p), b"aligned")):
        assert lib.uav_source_moments(h, *args, None) == 2 and what in lib.uav_last_error(), (what, lib.uav_last_error())
    st = C.c_void_p(a.data_ptr() + 8 * 1024)
    assert lib.uav_source_moments(h, p, p, p, 1, 1, 3, cfg(use_tke=False), None, st, None) == 0     # D = 3 is enough without obs[3]
    for args, what in (((None, 1, g, p, p), b"NULL"), ((p, 1, g, None, p), b"NULL"), ((p, 1, g, p, None), b"NULL"),
                       ((p, 1, None, p, p), b"NULL cfg"), ((p, 0, g, p, p), b"at least 1"),
                       ((p, 1, cfg(min_samples=3), p, p), b"min_samples"), ((p, 1, cfg(min_pivot=-1.0), p, p), b"min_pivot")):
        assert lib.uav_source_solve(h, *args, None) == 2 and what in lib.uav_last_error(), what
    for args, what in (((None, p, p, 1, 30.0, 100.0, 5.0, None, p), b"NULL"), ((p, None, p, 1, 30.0, 100.0, 5.0, None, p), b"NULL"),
                       ((p, p, None, 1, 30.0, 100.0, 5.0, None, p), b"NULL"), ((p, p, p, 1, 30.0, 100.0, 5.0, None, None), b"NULL"),
                       ((p, p, p, 0, 30.0, 100.0, 5.0, None, p), b"at least 1"), ((p, p, p, 1, 30.0, 100.0, nan, None, p), b"NaN")):
        assert lib.uav_source_summary(h, *args, None) == 2 and what in lib.uav_last_error(), what
    torch.cuda.synchronize()
