"""Anisotropic plumes: the field generator's plume term and the six-term source estimator (source_fit={"model": "aniso"}).

A plume stretched along the wind is an elliptical Gaussian centred on the source,
    base = peak exp(-(u^2 / 2 sigma_major^2 + v^2 / 2 sigma_minor^2)),  u, v = the offset from the source in the ellipse's frame,
and uav_plume_bank (csrc/source_aniso.hip) fills [F, 500, 500, 2] banks of clip(base + tke, 0, 100) with E3's turbulence; plume_base
states `base` in numpy.  A record of such a field still carries b = 100 obs[2] - 9 obs[3], and ln b is a full quadratic,
    ln b = a0 + a1 p + a2 q + a3 p^2 + a4 p q + a5 q^2,
linear in six parameters: the weighted least-squares fit of source_fit.py with two more terms gives the source, both widths, the
axis angle and the peak in closed form.  p, q, the centre, SCALE, b, w = b^2, which records are used, chunking, the `ended`
handling and the largest sample are source_fit.moments_chunk's.  Three kernels, none of which the host waits for:

  uav_source_moments6   per chunk of records: A (21), g (6), the count, the centre and the largest sample, per env
  uav_source_solve6     per evaluation: scaled Cholesky of the 6 x 6 system -> mu, sigma_major, sigma_minor, theta, peak, strength
  uav_source_summary6   sixteen sums against the true sources and, where given, the true widths, angle and peak per env

moments_chunk6, coefficients6, solve6 and summarise6 state them in numpy in the kernels' order of operations.  What is NOT in
here: a six-term stop scan (source_stop is four-term), plumes whose width grows downwind or that vanish upwind of the source.
"""
from __future__ import annotations

import numpy as np

from .source_fit import DEGENERATE, FEW, FITTED, NOT_A_PEAK, SCALE, SLOTS, TWO_PI, _block256, _tree, used_records

STATE_N, EST_N, SUM_N, PLUME_PARAM_N = 33, 10, 16, 8     # ops.SRC6_STATE_N, SRC6_EST_N, SRC6_SUM_N, PLUME_PARAM_N
N_PHI, N_A, N_ACC = 6, 21, 28                            # phi = (1, p, q, p p, p q, q q); count | A | g
ST_A, ST_G, ST_BMAX = 3, 24, 30
PI = 3.141592653589793
MIN_SAMPLES = 8                                          # the default of model="aniso"; six parameters: never below 6
# A's upper triangle by rows -> its place among the state's 21 entries
_IDX = [[0] * N_PHI for _ in range(N_PHI)]
_n = 0
for _i in range(N_PHI):
    for _j in range(_i, N_PHI):
        _IDX[_i][_j] = _IDX[_j][_i] = _n
        _n += 1
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
def fresh_state6(n):
    """state f64 [n, 33] of an evaluation that has not stepped yet: all zeros."""
    return np.zeros((n, STATE_N), np.float64)


def moments_chunk6(flags, obs, pos, state, ended=None, use_tke=True, background=0.0, floor=1.0, **_):
    """uav_source_moments6: the new state f64 [n, 33] after one chunk of records.  source_fit.moments_chunk with phi = (1, p, q,
    p p, p q, q q): A_ij = (w phi_i) phi_j for i <= j by rows, g_i = (w phi_i) ln b; the same order of summation."""
    used, b, cell = used_records(flags, obs, pos, ended, use_tke, background, floor)
    n, k = used.shape
    st = np.array(state, np.float64).reshape(n, STATE_N).copy()
    live = np.ones(n, bool) if ended is None else np.asarray(ended) == 0
    any_used = used.any(1)
    i0 = used.argmax(1)
    e = np.arange(n)
    new_c = live & any_used & ~(st[:, 0] > 0.0)                 # the centre: the cell of the env's first used record, then fixed
    st[new_c, 1] = cell[e, i0, 0][new_c].astype(np.float64)
    st[new_c, 2] = cell[e, i0, 1][new_c].astype(np.float64)
    p = (cell[:, :, 0].astype(np.float64) - st[:, 1:2]) / SCALE
    q = (cell[:, :, 1].astype(np.float64) - st[:, 2:3]) / SCALE
    bu = np.where(used, b, 1.0)
    w, lb = bu * bu, np.log(bu)
    phi = [np.ones_like(w), p, q, p * p, p * q, q * q]
    wphi = [w] + [w * phi[j] for j in range(1, N_PHI)]
    cols = [np.ones_like(w)]
    cols += [wphi[i] * phi[j] if j else wphi[i] for i in range(N_PHI) for j in range(i, N_PHI)]
    cols += [wphi[i] * lb for i in range(N_PHI)]
    c = np.where(used[:, :, None], np.stack(cols, 2), 0.0)
    nb = (k + 63) // 64
    c = np.concatenate([c, np.zeros((n, nb * 64 - k, N_ACC))], 1).reshape(n, nb, 64, N_ACC)
    acc = np.zeros((n, 64, N_ACC), np.float64)
    for blk in range(nb):
        acc = acc + c[:, blk]
    tot = _tree(acc)
    st[live, 0] = st[live, 0] + tot[live, 0]
    st[live, ST_A:ST_BMAX] = st[live, ST_A:ST_BMAX] + tot[live, 1:]
    im = np.where(used, b, -np.inf).argmax(1)                   # the first of equal largest
    bm = b[e, im]
    with np.errstate(invalid="ignore"):
        up = live & any_used & (bm > st[:, ST_BMAX])            # strictly: an earlier chunk's record wins a tie
    st[up, ST_BMAX] = bm[up]
    st[up, ST_BMAX + 1] = cell[e, im, 0][up].astype(np.float64)
    st[up, ST_BMAX + 2] = cell[e, im, 1][up].astype(np.float64)
    return st


def scaled_system6(state):
    """(S f64 [n, 6, 6], h f64 [n, 6], d f64 [n, 6]): A scaled by d_j = sqrt(A_jj) and g / d, the system solve6 factors."""
    st = np.asarray(state, np.float64).reshape(-1, STATE_N)
    A = np.stack([np.stack([st[:, ST_A + _IDX[i][j]] for j in range(N_PHI)], 1) for i in range(N_PHI)], 1)
    with np.errstate(all="ignore"):
        d = np.sqrt(np.stack([A[:, j, j] for j in range(N_PHI)], 1))
        S = A / (d[:, :, None] * d[:, None, :])
        h = st[:, ST_G:ST_G + N_PHI] / d
    return S, h, d


def coefficients6(state, min_pivot=1e-6):
    """(a f64 [n, 6], degenerate bool [n], smallest pivot f64 [n]): source_fit.coefficients on the 6 x 6 system -- the scaled Cholesky
    by columns, the two triangular solves and the unscaling, every t = t - L * z one after the other, no fused multiply-add."""
    S, h, d = scaled_system6(state)
    n, N = S.shape[0], N_PHI
    L = np.zeros((n, N, N), np.float64)
    bad = np.zeros(n, bool)
    low = np.full(n, np.inf)
    with np.errstate(all="ignore"):
        for j in range(N):
            s = S[:, j, j]
            for c in range(j):
                s = s - L[:, j, c] * L[:, j, c]
            bad |= ~(np.isfinite(s) & (s >= np.float64(min_pivot)))
            low = np.where(np.isfinite(s), np.minimum(low, s), -np.inf)
            L[:, j, j] = np.sqrt(s)
            for i in range(j + 1, N):
                t = S[:, i, j]
                for c in range(j):
                    t = t - L[:, i, c] * L[:, j, c]
                L[:, i, j] = t / L[:, j, j]
        z = np.zeros((n, N), np.float64)
        u = np.zeros((n, N), np.float64)
        for j in range(N):
            t = h[:, j]
            for c in range(j):
                t = t - L[:, j, c] * z[:, c]
            z[:, j] = t / L[:, j, j]
        for j in range(N - 1, -1, -1):
            t = z[:, j]
            for c in range(j + 1, N):
                t = t - L[:, c, j] * u[:, c]
            u[:, j] = t / L[:, j, j]
        a = u / d
    return a, bad, low


def solve6(state, min_samples=MIN_SAMPLES, min_pivot=1e-6, **_):
    """uav_source_solve6: (est f64 [n, 10], status u8 [n]).  est = {mu_x, mu_y, sigma_major, sigma_minor, theta, peak, strength,
    largest sample's x, y, b}; the first seven are NaN unless status is FITTED, all ten for a count of 0.  Lambda = -[[2 a3, a4],
    [a4, 2 a5]] is the plume's inverse covariance in units of SCALE cells: a peak iff det > 0 and trace > 0."""
    st = np.asarray(state, np.float64).reshape(-1, STATE_N)
    n = st.shape[0]
    est = np.full((n, EST_N), np.nan)
    status = np.zeros(n, np.uint8)
    count = st[:, 0]
    some = count > 0.0
    est[some, 7], est[some, 8], est[some, 9] = st[some, ST_BMAX + 1], st[some, ST_BMAX + 2], st[some, ST_BMAX]
    few = ~(count >= np.float64(min_samples))
    a, bad, _ = coefficients6(st, min_pivot)
    with np.errstate(all="ignore"):
        l11, l12, l22 = -(2.0 * a[:, 3]), -a[:, 4], -(2.0 * a[:, 5])
        det = l11 * l22 - l12 * l12
        trace = l11 + l22
        m0 = (l22 * a[:, 1] - l12 * a[:, 2]) / det
        m1 = (l11 * a[:, 2] - l12 * a[:, 1]) / det
        mx = st[:, 1] + SCALE * m0
        my = st[:, 2] + SCALE * m1
        hd = (l11 - l22) / 2.0
        disc = np.sqrt(hd * hd + l12 * l12)
        big = trace / 2.0 + disc
        small = det / big
        s_major = SCALE / np.sqrt(small)
        s_minor = SCALE / np.sqrt(big)
        th = np.arctan2(-(2.0 * l12), l22 - l11) / 2.0
        theta = np.where(th < 0.0, th + PI, th)
        peak = np.exp(a[:, 0] + (a[:, 1] * m0 + a[:, 2] * m1) / 2.0)
        strength = TWO_PI * (s_major * s_minor) * peak
        vals = (mx, my, s_major, s_minor, theta, peak, strength)
        peaked = np.isfinite(a).all(1) & (det > 0.0) & (trace > 0.0)
        for v in vals:
            peaked &= np.isfinite(v)
    status[:] = np.where(few, FEW, np.where(bad, DEGENERATE, np.where(peaked, FITTED, NOT_A_PEAK)))
    ok = status == FITTED
    for j, v in enumerate(vals):
        est[ok, j] = v[ok]
    return est, status


def summarise6(est, status, src, truth, loc_tol):
    """uav_source_summary6: dict(sums f64 [16], loc_err f64 [n]).  sums = {envs, fitted, few, degenerate, not a peak, sum of the
    fitted envs' errors, of their squares, how many within loc_tol | of the fitted envs whose truth row {sigma_major, sigma_minor,
    theta, peak} is finite: the sums of the relative errors of sigma_major and sigma_minor, of the angle error folded into
    [0, pi / 2], of the relative errors of the peak and of the strength 2 pi sigma_major sigma_minor peak | the sum of the largest
    samples' distances to the source, how many envs have one | how many fitted envs have a finite truth row}.  truth None: as all
    NaN.  source_fit.summarise's order of summation."""
    est, status = np.asarray(est, np.float64).reshape(-1, EST_N), np.asarray(status, np.uint8)
    src = np.asarray(src, np.float64)
    n = status.shape[0]
    tr = np.full((n, 4), np.nan) if truth is None else np.asarray(truth, np.float64).reshape(n, 4)
    fit = status == FITTED
    with np.errstate(all="ignore"):
        dx, dy = est[:, 0] - src[:, 0], est[:, 1] - src[:, 1]
        err = np.where(fit, np.sqrt(dx * dx + dy * dy), np.nan)
        within = fit & (err <= np.float64(loc_tol))
        known = fit & np.isfinite(tr).all(1)
        r1 = np.abs(est[:, 2] - tr[:, 0]) / tr[:, 0]
        r2 = np.abs(est[:, 3] - tr[:, 1]) / tr[:, 1]
        da = np.fmod(np.abs(est[:, 4] - tr[:, 2]), PI)
        da = np.where(da > PI / 2.0, PI - da, da)
        rp = np.abs(est[:, 5] - tr[:, 3]) / tr[:, 3]
        ts = TWO_PI * (tr[:, 0] * tr[:, 1]) * tr[:, 3]
        rs = np.abs(est[:, 6] - ts) / ts
        has = est[:, 9] == est[:, 9]
        mx, my = est[:, 7] - src[:, 0], est[:, 8] - src[:, 1]
        md = np.sqrt(mx * mx + my * my)
    z = np.zeros(n)
    vals = np.stack([fit.astype(np.float64), (status == FEW).astype(np.float64), (status == DEGENERATE).astype(np.float64),
                     (status == NOT_A_PEAK).astype(np.float64), np.where(fit, err, z), np.where(fit, err * err, z),
                     within.astype(np.float64), np.where(known, r1, z), np.where(known, r2, z), np.where(known, da, z),
                     np.where(known, rp, z), np.where(known, rs, z), np.where(has, md, z), has.astype(np.float64),
                     known.astype(np.float64)], axis=1)
    acc = np.zeros((SLOTS, SUM_N - 1), np.float64)
    for r0 in range(0, n, SLOTS):
        c = vals[r0:r0 + SLOTS]
        acc[:c.shape[0]] += c
    return {"sums": np.concatenate([[np.float64(n)], _block256(acc)]), "loc_err": err}


def fit_records6(chunks, n, ended_of=None, **cfg):
    """The statement over a whole episode, as source_fit.fit_records: chunks = [(flags, obs, pos)] in time order -> (state, est,
    status)."""
    from .eval_track import fresh_episodes, reduce_chunk
    from .source_fit import check_source_fit
    cfg = check_source_fit(**{"model": "aniso", **cfg})
    st, ep, t0 = fresh_state6(n), fresh_episodes(n), 0
    for i, (flags, obs, pos) in enumerate(chunks):
        ended = ep[1] if ended_of is None else ended_of(i)
        st = moments_chunk6(flags, obs, pos, st, ended, **cfg)
        ep = reduce_chunk(flags, obs, pos, t0, *ep)
        t0 += np.asarray(flags).shape[1]
    est, status = solve6(st, **cfg)
    return st, est, status


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


# ------------------------------------------------------------------------------------------ the device side
class SourceFitAniso:
    """SourceFit's interface on the six-term kernels: restart(), chunk(recs, ended) once per chunk of greedy records BEFORE that
    chunk's uav_greedy_reduce, finish(src, truth) after the last.  Launches only: nothing is read by the host."""

    def __init__(self, n, device="cuda", **cfg):
        import torch
        from . import ops
        from .source_fit import check_source_fit
        self.cfg = check_source_fit(**{"model": "aniso", **cfg})
        self.n, self.device = int(n), torch.device(device)
        self._c = ops.source_fit_cfg(**self.cfg)
        self.state = torch.zeros(self.n, STATE_N, dtype=torch.float64, device=self.device)
        self.est = torch.zeros(self.n, EST_N, dtype=torch.float64, device=self.device)
        self.status = torch.zeros(self.n, dtype=torch.uint8, device=self.device)
        self.loc_err = torch.zeros(self.n, dtype=torch.float64, device=self.device)
        self.sums = torch.zeros(SUM_N, dtype=torch.float64, device=self.device)

    def restart(self):
        self.state.zero_()

    def chunk(self, recs, ended=None):
        """ended u8 [n]: ep_state as it stands before this chunk's uav_greedy_reduce, or None (nothing has ended)."""
        from . import ops
        ops.source_moments6(recs, self._c, self.state, ended)

    def finish(self, src, truth=None, loc_tol=None, sums=None):
        """uav_source_solve6, then uav_source_summary6 against src f64 [n, 2] and truth f64 [n, 4] or None into `sums` (default:
        self.sums); returns it."""
        from . import ops
        ops.source_solve6(self.state, self._c, self.est, self.status)
        return ops.source_summary6(self.est, self.status, src, truth, self.cfg["loc_tol"] if loc_tol is None else loc_tol,
                                   self.sums if sums is None else sums, loc_err=self.loc_err)

    def metrics(self):
        """evaluate()'s source_* entries as numpy arrays.  Waits for the device."""
        return metrics6(self.est.cpu().numpy(), self.status.cpu().numpy(), self.loc_err.cpu().numpy())
