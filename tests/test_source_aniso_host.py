"""CPU: the numpy statement of the six-term source estimator and of the anisotropic plume term (uavppo/source_aniso.py) -- recovery of
the truth on clean anisotropic walkers where the four-term fit is off by cells, agreement with the four-term fit on round plumes,
the solve against numpy.linalg.lstsq, chunk invariance, every status from a constructed case, option parsing, bank specs."""
import json
import os

import numpy as np
import pytest

from _source_aniso_cases import EXPECTED, K, MIN_K, clean_walkers, episodes6, estimates6
from _source_fit_cases import episodes
from conftest import ROOT


@pytest.fixture(scope="module")
def sa():
    from uavppo import source_aniso
    return source_aniso


@pytest.fixture(scope="module")
def sf():
    from uavppo import source_fit
    return source_fit


@pytest.fixture(scope="module")
def clean(sa, sf):
    ep = clean_walkers()
    n = ep["src"].shape[0]
    chunks = [(ep["flags"], ep["obs"], ep["pos"])]
    return ep, sa.fit_records6(chunks, n), sf.fit_records(chunks, n)


def bits64(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def _errors(est, ep):
    tr = ep["truth"]
    da = np.abs(est[:, 4] - tr[:, 2])
    return {"location_cells": np.hypot(est[:, 0] - ep["src"][:, 0], est[:, 1] - ep["src"][:, 1]),
            "sigma_major_rel": np.abs(est[:, 2] - tr[:, 0]) / tr[:, 0], "sigma_minor_rel": np.abs(est[:, 3] - tr[:, 1]) / tr[:, 1],
            "theta_rad": np.minimum(da, np.pi - da), "peak_rel": np.abs(est[:, 5] - tr[:, 3]) / tr[:, 3],
            "strength_rel": np.abs(est[:, 6] / (2.0 * np.pi * tr[:, 0] * tr[:, 1] * tr[:, 3]) - 1.0)}


def test_six_term_fit_recovers_a_stretched_plume(sa, clean):
    """400 episodes of 48 records, walkers at 0.5 .. 2 sigma in the ellipse's frame, ratio 1.5 .. 3, major sigma 20 .. 45.  The
    bounds are set 10 .. 40 x above a numpy prototype's maxima (location 8.9e-7 cells, widths / peak 2.4e-8, angle 2.5e-8 rad,
    strength 1.8e-8, smallest pivot 2.9e-3).  The committed statement's own maxima are in profiles/source_aniso_accuracy.json."""
    ep, (st, est, status), _ = clean
    assert (status == 0).all()
    err = _errors(est, ep)
    print({k: float(v.max()) for k, v in err.items()})
    assert err["location_cells"].max() <= 1e-5
    for key in ("sigma_major_rel", "sigma_minor_rel", "peak_rel", "strength_rel"):
        assert err[key].max() <= 1e-6, key
    assert err["theta_rad"].max() <= 1e-6
    _, bad, low = sa.coefficients6(st)
    print("smallest pivot", float(low.min()))
    assert not bad.any() and low.min() >= 100 * 1e-6
    prof = json.load(open(os.path.join(ROOT, "profiles", "source_aniso_accuracy.json")))["six_term_max"]
    for key, v in err.items():                                 # the committed figures are this statement's (numpy's libm may differ in a last bit)
        assert np.isclose(prof[key], v.max(), rtol=0.05, atol=0.0), key


def test_four_term_fit_is_off_by_cells_on_the_same_records(clean):
    """The case the six-term model exists for: a round-plume fit of a stretched plume misplaces the source."""
    ep, _, (_, est4, status4) = clean
    err4 = np.hypot(est4[:, 0] - ep["src"][:, 0], est4[:, 1] - ep["src"][:, 1])
    print("four-term median / max", float(np.nanmedian(err4)), float(np.nanmax(err4)))
    assert (status4 == 0).mean() > 0.9 and np.nanmedian(err4) > 0.5


def test_six_term_fit_agrees_with_the_four_term_fit_on_round_plumes(sa, sf):
    """tests/_source_fit_cases.py's isotropic records: both widths and mu equal the four-term answer (1e-6 relative, 1e-6 cells);
    the angle of a circle means nothing and is not compared.  Both fits ask for 12 records, twice the six parameters: the records
    are f32, and the two models answer that rounding differently -- with 9 records (three more than parameters) the six-term mu
    of one env here moves 1.2e-6 cells from the four-term one, both being 1 .. 2e-6 cells from the true source."""
    ep = episodes(240, 64, 6)
    st4 = sf.moments_chunk(ep["flags"], ep["obs"], ep["pos"], ep["state"], ep["ended"])
    start = np.zeros((240, sa.STATE_N))
    st6 = sa.moments_chunk6(ep["flags"], ep["obs"], ep["pos"], start, ep["ended"])
    est4, s4 = sf.solve(st4, min_samples=12)
    est6, s6 = sa.solve6(st6, min_samples=12)
    both = (s4 == 0) & (s6 == 0) & (ep["ended"] == 0)
    assert both.sum() >= 80
    assert (np.abs(est6[both, 0:2] - est4[both, 0:2]) <= 1e-6).all()
    for j in (2, 3):
        assert (np.abs(est6[both, j] - est4[both, 2]) <= 1e-6 * est4[both, 2]).all()
    assert (np.abs(est6[both, 5] - est4[both, 3]) <= 1e-6 * est4[both, 3]).all()


def test_coefficients6_is_the_weighted_least_squares_solution(sa, sf):
    ep = clean_walkers(n=40, seed=3)
    st = sa.moments_chunk6(ep["flags"], ep["obs"], ep["pos"], sa.fresh_state6(40))
    a, bad, _ = sa.coefficients6(st)
    assert not bad.any()
    used, b, cell = sf.used_records(ep["flags"], ep["obs"], ep["pos"])
    for e in range(40):
        u = used[e]
        p, q = (cell[e, u, 0] - st[e, 1]) / 32.0, (cell[e, u, 1] - st[e, 2]) / 32.0
        X = np.stack([np.ones_like(p), p, q, p * p, p * q, q * q], 1)
        want = np.linalg.lstsq(X * b[e, u, None], b[e, u] * np.log(b[e, u]), rcond=None)[0]      # sqrt(w) = b
        assert np.allclose(a[e], want, rtol=1e-6, atol=1e-8), e


@pytest.mark.parametrize("k", [65, 130])
def test_moments_chunk6_does_not_depend_on_the_chunking(sa, k):
    """One chunk against the same records in two and three chunks, as for the four-term statement: the count, the centre and the
    largest sample are the same bits; A and g are sums in another order (each chunk through its own lanes and tree)."""
    from uavppo import eval_track as et
    ep = episodes6(36, k, 6, seed=1)
    f, o, p = ep["flags"], ep["obs"], ep["pos"]
    one = sa.moments_chunk6(f, o, p, ep["state"], ep["ended"])

    def pieces(cuts):
        st, e, t0 = ep["state"], (np.zeros(36, np.int32), ep["ended"].copy(), np.zeros((36, 2))), 0
        for a, b in zip((0,) + cuts, cuts + (k,)):
            nxt = et.reduce_chunk(f[:, a:b], o[:, a:b], p[:, a:b], t0, *e)
            st = sa.moments_chunk6(f[:, a:b], o[:, a:b], p[:, a:b], st, e[1])
            e, t0 = nxt, b
        return st
    exact = [0, 1, 2, 30, 31, 32]                              # the count, the centre, the largest sample
    tol = (k + 8) * 2.0 ** -52 * np.abs(one[:, 3:30]).max(1, keepdims=True)      # A, g: (records + 8) eps of the row's largest sum
    for cuts in ((64,), (64, 128))[:1 if k < 129 else 2]:
        got = pieces(cuts)
        assert np.array_equal(bits64(got[:, exact]), bits64(one[:, exact]))
        assert (np.abs(got - one) <= tol).all()
    for cuts in ((31,), (20, 50)):
        got = pieces(cuts)
        assert np.array_equal(bits64(got[:, exact]), bits64(one[:, exact]))
        assert (np.abs(got - one) <= tol).all()


def test_every_status_from_a_constructed_case(sa):
    """A straight track is DEGENERATE, a saddle and a bowl are NOT_A_PEAK, 5 usable records are FEW (min_samples 8), 0 records leave
    all ten estimates NaN; an env that comes in ended keeps its state to the bit."""
    n, k = 48, MIN_K
    ep = episodes6(n, k, 6)
    st = sa.moments_chunk6(ep["flags"], ep["obs"], ep["pos"], ep["state"], ep["ended"])
    gone = ep["ended"] != 0
    assert np.array_equal(bits64(st[gone]), bits64(ep["state"][gone]))
    est, status = sa.solve6(st)
    for e in range(n):
        if EXPECTED[e % K] is not None:
            assert status[e] == EXPECTED[e % K], (e, ep["kind"][e], status[e])
    assert (st[ep["kind"] == 8, 0] == 5).all() and (st[ep["kind"] == 9, 0] == 8).all() and (st[ep["kind"] == 7, 0] == 0).all()
    assert np.isnan(est[ep["kind"] == 7]).all()
    fit = (status == 0) & ~gone
    assert np.isnan(est[(status != 0) & ~gone][:, 0:7]).all() and np.isfinite(est[fit]).all()
    assert ((est[fit, 4] >= 0.0) & (est[fit, 4] < np.pi)).all() and (est[fit, 2] >= est[fit, 3]).all()
    live = fit & np.isin(ep["kind"], (0, 1, 2, 9, 11))
    assert (np.hypot(*(est[live, 0:2] - ep["src"][live]).T) <= 1e-3).all()


def test_summarise6_counts_and_truth_rows(sa):
    est, status, src, truth = estimates6(300)
    S = sa.summarise6(est, status, src, truth, 5.0)["sums"]
    fit = status == 0
    known = fit & np.isfinite(truth).all(1)
    assert S[0] == 300 and S[1] == fit.sum() and S[15] == known.sum() and 0 < known.sum() < fit.sum()
    assert np.isclose(S[8], (np.abs(est[known, 2] - truth[known, 0]) / truth[known, 0]).sum())
    da = np.abs(est[known, 4] - truth[known, 2])
    assert np.isclose(S[10], np.minimum(da, np.pi - da).sum()) and (np.minimum(da, np.pi - da) <= np.pi / 2).all()
    none = sa.summarise6(est, status, src, None, 5.0)["sums"]
    assert (none[8:13] == 0).all() and none[15] == 0 and np.array_equal(none[:8], S[:8]) and np.array_equal(none[13:15], S[13:15])
    row = sa.source_row6(S)
    from uavppo import eval_track as et, source_fit as sf
    cols = et.curve_columns(source=True, aniso=True)
    assert cols[-9:] == sf.SOURCE_COLUMNS + sa.SOURCE_COLUMNS6 and et.curve_columns(source=True) == cols[:-3]
    assert len(row) == 9 and row[0] == S[1] / 300 and np.isclose(row[3], S[8] / S[15]) and np.isclose(row[6], S[9] / S[15])
    assert np.isclose(row[7], S[10] / S[15]) and np.isclose(row[8], S[12] / S[15]) and np.isclose(row[5], S[13] / S[14])
    blind = sa.source_row6(none)
    assert blind[:3] == row[:3] and blind[5] == row[5] and all(np.isnan(blind[j]) for j in (3, 4, 6, 7, 8))
    assert len(et.curve_row(3, np.arange(8.0) + 1, np.zeros(7), S)) == len(cols)


def test_model_option_and_its_refusals(sa, sf):
    iso = sf.check_source_fit()
    assert "model" not in iso and iso["min_samples"] == 5 and not sf.is_aniso(iso) and not sf.is_aniso(None)
    assert sf.check_source_fit(model="iso") == iso
    an = sf.check_source_fit(model="aniso")
    assert an["model"] == "aniso" and an["min_samples"] == 8 and sf.is_aniso(an)
    assert {k: v for k, v in an.items() if k not in ("model", "min_samples")} == {k: v for k, v in iso.items() if k != "min_samples"}
    assert sf.check_source_fit(model="aniso", min_samples=6)["min_samples"] == 6
    assert sf.option({"model": "aniso"}) == an
    for kw, what in ((dict(model="aniso", min_samples=5), "min_samples"), (dict(model="round"), "model"), (dict(model=None), "model"),
                     (dict(model="aniso", floor=-1.0), "floor"), (dict(min_samples=3), "min_samples")):
        with pytest.raises(ValueError, match=what):
            sf.check_source_fit(**kw)
    with pytest.raises(ValueError, match="min_samples"):
        sa.fit_records6([], 4, min_samples=4)


def test_plume_params_and_their_refusals(sa):
    P = sa.plume_params([[100.0, 200.0]], 30.0, 12.0, 0.7, 90.0)
    assert P.shape == (1, sa.PLUME_PARAM_N) and P[0, 4] == np.cos(0.7) and P[0, 5] == np.sin(0.7) and P[0, 7] == 0.7
    assert sa.check_plume_params(P) is not None
    # the peak at the source, the major axis' one-sigma point at exp(-1/2)
    assert sa.plume_base(P[0], 100.0, 200.0) == 90.0
    x, y = 100.0 + 30.0 * np.cos(0.7), 200.0 + 30.0 * np.sin(0.7)
    assert np.isclose(sa.plume_base(P[0], x, y), 90.0 * np.exp(-0.5), rtol=1e-12)
    x, y = 100.0 - 12.0 * np.sin(0.7), 200.0 + 12.0 * np.cos(0.7)
    assert np.isclose(sa.plume_base(P[0], x, y), 90.0 * np.exp(-0.5), rtol=1e-12)
    assert sa.plume_base(P[0], 499.0, 0.0) == 0.0                                  # e > 300
    for j, v, what in ((0, np.nan, "non-finite"), (2, 0.0, "sigma"), (3, -1.0, "sigma"), (6, 0.0, "peak"), (4, 0.5, "cos"),
                       (7, np.inf, "non-finite")):
        bad = P.copy()
        bad[0, j] = v
        with pytest.raises(ValueError, match=what):
            sa.check_plume_params(bad)
    with pytest.raises(ValueError, match="expected"):
        sa.check_plume_params(np.zeros((0, 8)))


def test_aniso_bank_specs():
    from uavppo import field_bank as fb
    assert fb.parse_aniso("aniso:8") == (8, None) and fb.parse_aniso("aniso:3:1.2-4") == (3, (1.2, 4.0))
    for bad in ("aniso:", "aniso:0", "aniso:x", "aniso:4:3", "aniso:4:3-2", "aniso:4:0.5-2", "aniso:4:1-2:3", "synth:4"):
        with pytest.raises(ValueError, match="aniso:F"):
            fb.parse_aniso(bad)
    for kw, what in ((dict(sigma=(0.0, 10.0)), "sigma"), (dict(ratio=(0.5, 2.0)), "ratio"), (dict(peak=(50.0, 40.0)), "peak"),
                     (dict(n_fields=0), "n_fields")):
        with pytest.raises(ValueError, match=what):
            fb.synthesise_aniso(**{"n_fields": 2, "device": "cpu", **kw})
    assert fb.load_with_truth(None) == (None, None, None)


def test_npz_banks_carry_an_optional_truth(tmp_path):
    import torch
    from uavppo import field_bank as fb
    rng = np.random.default_rng(0)
    bank = torch.from_numpy(rng.uniform(0.0, 100.0, (2, 500, 500, 2)))
    src = torch.tensor([[100.0, 200.0], [300.0, 50.0]], dtype=torch.float64)
    truth = torch.tensor([[30.0, 12.0, 0.7, 90.0], [25.0, 10.0, 2.0, 100.0]], dtype=torch.float64)
    fb.save_npz(str(tmp_path / "a.npz"), bank, src, truth)
    fb.save_npz(str(tmp_path / "b.npz"), bank, src)
    b, s, t = fb.load_with_truth(str(tmp_path / "a.npz"), device="cpu")
    assert torch.equal(b, bank) and torch.equal(s, src) and torch.equal(t, truth)
    assert fb.load_with_truth(str(tmp_path / "b.npz"), device="cpu")[2] is None
    b2, s2 = fb.load(str(tmp_path / "a.npz"), device="cpu")
    assert torch.equal(b2, bank) and torch.equal(s2, src)


def test_source_estimates_csv_gains_two_columns_for_this_model_only(sa, sf, tmp_path):
    est, status, _, _ = estimates6(5)
    m6 = sa.metrics6(est, status, np.full(5, 1.5))
    sf.write_estimates(str(tmp_path / "six.csv"), m6)
    four = {k: v for k, v in m6.items() if k not in ("source_sigma_minor", "source_theta")}
    sf.write_estimates(str(tmp_path / "four.csv"), four)
    six_lines, four_lines = open(tmp_path / "six.csv").read().splitlines(), open(tmp_path / "four.csv").read().splitlines()
    assert four_lines[0].split(",") == sf.ESTIMATE_COLUMNS
    head = six_lines[0].split(",")
    assert head[:5] == sf.ESTIMATE_COLUMNS[:5] and head[5:7] == sa.ESTIMATE_COLUMNS6 and head[7:] == sf.ESTIMATE_COLUMNS[5:]
    row6, row4 = six_lines[1].split(","), four_lines[1].split(",")
    assert row6[:5] + row6[7:] == row4 and float(row6[5]) == est[0, 3] and float(row6[6]) == est[0, 4]
