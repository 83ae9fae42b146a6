"""Anisotropic plumes: the field generator's plume term and the six-term source estimator (source_fit={"model": "aniso"}).

A plume stretched along the wind is an elliptical Gaussian centred on the source,
    base = peak exp(-(u^2 / 2 sigma_major^2 + v^2 / 2 sigma_minor^2)),  u, v = the offset from the source in the ellipse's frame,
and uav_plume_bank (csrc/source_aniso.hip) fills [F, 500, 500, 2] banks of clip(base + tke, 0, 100) with E3's turbulence; plume_base
states `base` in numpy.  A record of such a field still carries b = 100 obs[2] - 9 obs[3], and ln b is a full quadratic,
    ln b = a0 + a1 p + a2 q + a3 p^2 + a4 p q + a5 q^2,
linear in six parameters: the weighted least-squares fit of source_fit.py with two more terms gives the source, both widths, the
axis angle and the peak in closed form.  The moments, the Cholesky and the solve are source_fit's own, given the basis ANISO; what
is stated here is the six-term closed form and the summary's truth columns.  Three kernels, none of which the host waits for:

  uav_source_moments6   per chunk of records: A (21), g (6), the count, the centre and the largest sample, per env
  uav_source_solve6     per evaluation: scaled Cholesky of the 6 x 6 system -> mu, sigma_major, sigma_minor, theta, peak, strength
  uav_source_summary6   sixteen sums against the true sources and, where given, the true widths, angle and peak per env

moments_chunk6, coefficients6, solve6 and summarise6 state them in numpy in the kernels' order of operations (SourceFit(model="aniso")
of source_fit.py drives them on the device).  What is NOT in
here: a six-term stop scan (source_stop is four-term), plumes whose width grows downwind or that vanish upwind of the source.
"""
from __future__ import annotations

import numpy as np

from . import source_fit as sf
from .source_fit import ANISO, SCALE, TWO_PI

STATE_N, EST_N, SUM_N, PLUME_PARAM_N = ANISO.state_n, ANISO.est_n, ANISO.sum_n, 8     # ops.SRC6_STATE_N, SRC6_EST_N, SRC6_SUM_N, PLUME_PARAM_N
PI = 3.141592653589793
MIN_SAMPLES = ANISO.min_samples                          # the default of model="aniso"; six parameters: never below 6
SOURCE_COLUMNS6 = ["Mean_Sigma_Minor_Rel_Error", "Mean_Theta_Error", "Mean_Strength_Rel_Error"]
ESTIMATE_COLUMNS6 = ["Sigma_Minor", "Theta"]


# ------------------------------------------------------------------------------------------ the field
def plume_params(sources, sigma_major, sigma_minor, theta, peak):
    """params f64 [F, 8] of uav_plume_bank: {sx, sy, sigma_major, sigma_minor, cos theta, sin theta, peak, theta}; the host's cos / sin."""
    src = np.asarray(sources, np.float64).reshape(-1, 2)
    cols = [np.broadcast_to(np.asarray(v, np.float64), (src.shape[0],)) for v in (sigma_major, sigma_minor, theta, peak)]
    return np.stack([src[:, 0], src[:, 1], cols[0], cols[1], np.cos(cols[2]), np.sin(cols[2]), cols[3], cols[2]], 1)


def check_plume_params(params):
    """uav_plume_bank's refusals, as a ValueError with the reason; returns params as f64 [F, 8]."""
    P = np.asarray(params, np.float64)
    if P.ndim != 2 or P.shape[1] != PLUME_PARAM_N or P.shape[0] < 1:
        raise ValueError(f"plume params: expected [F >= 1, {PLUME_PARAM_N}], got {P.shape}")
    if not np.isfinite(P).all():
        raise ValueError("plume params: non-finite values")
    if not ((P[:, 2] > 0.0) & (P[:, 3] > 0.0)).all():
        raise ValueError("plume params: sigma_major and sigma_minor must be positive")
    if not (P[:, 6] > 0.0).all():
        raise ValueError("plume params: peak must be positive")
    if not (np.abs(P[:, 4] * P[:, 4] + P[:, 5] * P[:, 5] - 1.0) <= 1e-12).all():
        raise ValueError("plume params: cos^2 + sin^2 differs from 1 by more than 1e-12")
    return P


def plume_base(params, x, y):
    """The plume term of uav_plume_bank at cells x, y (arrays that broadcast) for ONE row of params, in the kernel's order of
    operations; exp is numpy's (the kernel's table-driven one agrees to 1e-15 absolute times the peak)."""
    sx, sy, s1, s2, cs, sn, peak = (np.float64(v) for v in np.asarray(params, np.float64)[:7])
    dx, dy = np.asarray(x, np.float64) - sx, np.asarray(y, np.float64) - sy
    u = dx * cs + dy * sn
    v = dy * cs - dx * sn
    e = u * u / (2.0 * (s1 * s1)) + v * v / (2.0 * (s2 * s2))
    return np.where(e <= 300.0, peak * np.exp(-np.minimum(e, 300.0)), 0.0)


# ------------------------------------------------------------------------------------------ the numpy definitions
# moments, Cholesky and solve are source_fit's, written once for any basis: these are its bindings to ANISO
def fresh_state6(n):
    """state f64 [n, 33] of an evaluation that has not stepped yet: all zeros."""
    return sf.fresh_state(n, ANISO)


def moments_chunk6(flags, obs, pos, state, ended=None, **cfg):
    """uav_source_moments6: source_fit.moments_chunk with phi = (1, p, q, p p, p q, q q)."""
    return sf.moments_chunk(flags, obs, pos, state, ended, **dict(cfg, basis=ANISO))


def scaled_system6(state):
    return sf.scaled_system(state, ANISO)


def coefficients6(state, min_pivot=1e-6):
    """(a f64 [n, 6], degenerate bool [n], smallest pivot f64 [n]): source_fit.cholesky on the 6 x 6 system."""
    return sf.cholesky(state, min_pivot, ANISO)


def closed_form6(a, cx, cy):
    """ANISO's closed form: a0 .. a5 and the centre -> ((mu_x, mu_y, sigma_major, sigma_minor, theta, peak, strength), peaked).
    Lambda = -[[2 a3, a4], [a4, 2 a5]] is the plume's inverse covariance in units of SCALE cells: a peak iff det > 0 and trace > 0
    (and every value finite)."""
    l11, l12, l22 = -(2.0 * a[:, 3]), -a[:, 4], -(2.0 * a[:, 5])
    det = l11 * l22 - l12 * l12
    trace = l11 + l22
    m0 = (l22 * a[:, 1] - l12 * a[:, 2]) / det
    m1 = (l11 * a[:, 2] - l12 * a[:, 1]) / det
    hd = (l11 - l22) / 2.0
    disc = np.sqrt(hd * hd + l12 * l12)
    big = trace / 2.0 + disc
    small = det / big
    s_major = SCALE / np.sqrt(small)
    s_minor = SCALE / np.sqrt(big)
    th = np.arctan2(-(2.0 * l12), l22 - l11) / 2.0
    theta = np.where(th < 0.0, th + PI, th)
    peak = np.exp(a[:, 0] + (a[:, 1] * m0 + a[:, 2] * m1) / 2.0)
    vals = (cx + SCALE * m0, cy + SCALE * m1, s_major, s_minor, theta, peak, TWO_PI * (s_major * s_minor) * peak)
    peaked = np.isfinite(a).all(1) & (det > 0.0) & (trace > 0.0)
    for v in vals:
        peaked &= np.isfinite(v)
    return vals, peaked


def solve6(state, min_samples=MIN_SAMPLES, min_pivot=1e-6, **_):
    """uav_source_solve6: (est f64 [n, 10], status u8 [n]).  est = {mu_x, mu_y, sigma_major, sigma_minor, theta, peak, strength,
    largest sample's x, y, b}; the first seven are NaN unless status is FITTED, all ten for a count of 0."""
    return sf.solve(state, min_samples, min_pivot, ANISO)


def summarise6(est, status, src, truth, loc_tol):
    """uav_source_summary6: dict(sums f64 [16], loc_err f64 [n]).  sums = {envs, fitted, few, degenerate, not a peak, sum of the
    fitted envs' errors, of their squares, how many within loc_tol | of the fitted envs whose truth row {sigma_major, sigma_minor,
    theta, peak} is finite: the sums of the relative errors of sigma_major and sigma_minor, of the angle error folded into
    [0, pi / 2], of the relative errors of the peak and of the strength 2 pi sigma_major sigma_minor peak | the sum of the largest
    samples' distances to the source, how many envs have one | how many fitted envs have a finite truth row}.  truth None: as all
    NaN.  source_fit.summary_sums' order of summation."""
    def truth_columns(est, fit):
        n = len(fit)
        tr = np.full((n, 4), np.nan) if truth is None else np.asarray(truth, np.float64).reshape(n, 4)
        known = fit & np.isfinite(tr).all(1)
        r1 = np.abs(est[:, 2] - tr[:, 0]) / tr[:, 0]
        r2 = np.abs(est[:, 3] - tr[:, 1]) / tr[:, 1]
        da = np.fmod(np.abs(est[:, 4] - tr[:, 2]), PI)
        da = np.where(da > PI / 2.0, PI - da, da)
        rp = np.abs(est[:, 5] - tr[:, 3]) / tr[:, 3]
        ts = TWO_PI * (tr[:, 0] * tr[:, 1]) * tr[:, 3]
        rs = np.abs(est[:, 6] - ts) / ts
        return [np.where(known, v, 0.0) for v in (r1, r2, da, rp, rs)], [known.astype(np.float64)]
    return sf.summary_sums(ANISO, est, status, src, loc_tol, truth_columns)


def fit_records6(chunks, n, ended_of=None, **cfg):
    """The statement over a whole episode: source_fit.fit_records with model "aniso"."""
    return sf.fit_records(chunks, n, ended_of, **{"model": "aniso", **cfg})


def source_row6(sums):
    """The nine eval_curve.csv columns of the six-term model from the sixteen sums: source_fit.SOURCE_COLUMNS (the sigma column is
    the major width's) and SOURCE_COLUMNS6.  Plain python numbers; NaN where nothing was fitted, the truth columns where no fitted
    env has a finite truth row."""
    S = np.asarray(sums, np.float64)
    n, fit, has, known = float(S[0]), float(S[1]), float(S[14]), float(S[15])
    nan = float("nan")

    def over(j, d):
        return float(S[j]) / d if d > 0 else nan
    return [over(1, n), over(5, fit), over(7, fit), over(8, known), over(11, known), over(13, has), over(9, known), over(10, known),
            over(12, known)]


def metrics6(est, status, loc_err):
    """evaluate()'s source_* entries from numpy est [N, 10], status [N], loc_err [N]: source_fit.metrics' keys (source_sigma is the
    major width) and source_sigma_minor, source_theta."""
    est = np.asarray(est, np.float64)
    return {"source_estimate": est[:, 0:2].copy(), "source_sigma": est[:, 2].copy(), "source_sigma_minor": est[:, 3].copy(),
            "source_theta": est[:, 4].copy(), "source_peak": est[:, 5].copy(), "source_strength": est[:, 6].copy(),
            "source_status": np.asarray(status, np.uint8).copy(), "source_error": np.asarray(loc_err, np.float64).copy(),
            "source_max_sample": est[:, 7:10].copy()}


def field_index(n_env, episode, n_fields, env_offset=0, n_env_total=None):
    """The field of each env's current episode, csrc/env_core.h: (global env + episode * total envs) mod F.  episode: an i32 / i64
    tensor [n_env] on the device; returns an i64 tensor there.  Torch indexing only: no host read."""
    import torch
    total = int(n_env_total) if n_env_total else int(n_env)
    e = torch.arange(int(n_env), dtype=torch.int64, device=episode.device) + int(env_offset)
    return (e + episode.to(torch.int64) * total) % int(n_fields)


def gather_truth(bank_truth, env):
    """truth f64 [N, 4] of the envs' CURRENT episodes from bank_truth f64 [F, 4] (device tensor, numpy or None -> None), by
    field_index on the env's episode counters: launches only.  Call it where the sources handed to the summary are taken."""
    import torch
    if bank_truth is None:
        return None
    if env.bank is None:
        raise ValueError("bank_truth: the env has no field bank the rows could belong to")
    bt = torch.as_tensor(bank_truth, dtype=torch.float64).to(env.device)
    if bt.ndim != 2 or tuple(bt.shape) != (env.bank.shape[0], 4):
        raise ValueError(f"bank_truth: expected [F = {env.bank.shape[0]}, 4] = {{sigma_major, sigma_minor, theta, peak}}, got {tuple(bt.shape)}")
    episode = env.peek()[3]
    return bt[field_index(env.num_envs, episode, bt.shape[0], env.env_offset, env.n_env_total)].contiguous()
