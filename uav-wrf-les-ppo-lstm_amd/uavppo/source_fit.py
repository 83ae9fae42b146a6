"""Where the measurements of a greedy episode say the plume's source is (evaluate(source_fit=...), EvalTracker(source_fit=...)).

The field the env samples (csrc/env_core.h field_at) is 100 exp(-d^2 / 2 sigma^2) + tke, clipped to 0 .. 100, and an observation
carries conc / 100 (obs[2]) and tke / 9 (obs[3]) of the same cell.  The plume term b = 100 obs[2] - 9 obs[3] is therefore known per
record, and ln b = a0 + a1 p + a2 q + a3 (p^2 + q^2) is linear in its four parameters: a weighted least-squares fit per env (Guo's
weighting w = b^2, which undoes the logarithm's emphasis on the far tail) gives the source, the width and the peak in closed form.
Three kernels (csrc/source_fit.hip), none of which the host waits for:

  uav_source_moments   per chunk of records: the normal equations A, g, the count, the centre and the largest sample, per env
  uav_source_solve     per evaluation: scaled Cholesky -> mu, sigma, peak, strength and a status per env
  uav_source_summary   twelve sums against the true sources, in uav_greedy_summary's order of summation

moments_chunk, solve and summarise state them in numpy, in the kernels' order of operations (chunking included): what the kernels
are tested against bit for bit.  Estimates during the episode, and the estimator as a stop rule, are in source_stop.py
(uav_source_stop_scan).  Anisotropic plumes: source_aniso.py (model="aniso").  What is NOT in here: a nonlinear refinement of the closed form, stop controllers replayed on the host (their hits are not in the flags).
"""
from __future__ import annotations

import numpy as np

STATE_N, EST_N, SUM_N = 20, 8, 12            # ops.SRC_STATE_N, SRC_EST_N, SRC_SUM_N
FITTED, FEW, DEGENERATE, NOT_A_PEAK = 0, 1, 2, 3
SLOTS = 256                                  # threads of uav_source_summary's one block
SCALE = 32.0                                 # p = (x - cx) / SCALE: exact in f64
TWO_PI = 6.283185307179586
# A's upper triangle by rows -> its place among the state's ten entries
_IDX = ((0, 1, 2, 3), (1, 4, 5, 6), (2, 5, 7, 8), (3, 6, 8, 9))
SOURCE_COLUMNS = ["Fit_Rate", "Mean_Source_Error", "Within_Tol_Rate", "Mean_Sigma_Rel_Error", "Mean_Peak_Rel_Error",
                  "Mean_Max_Sample_Error"]
ESTIMATE_FILE = "source_estimates.csv"
ESTIMATE_COLUMNS = ["Episode", "Status", "Est_X", "Est_Y", "Sigma", "Peak", "Strength", "Error", "Max_X", "Max_Y", "Max_B"]


def _num(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_))


def check_source_fit(use_tke=True, min_samples=None, background=0.0, floor=1.0, min_pivot=1e-6, loc_tol=5.0, model="iso"):
    """The estimator's keywords, refused with the reason (ValueError); returns them as a dict of plain values.  Pure host arithmetic.
    use_tke: subtract the record's own turbulence channel (else the constant `background`); a record is used iff b > floor and its
    cell was not clipped -- a floor near 0 lets the fit extrapolate from the far tail; min_samples >= 4 used records for a fit;
    min_pivot: the smallest accepted pivot of the scaled Cholesky; loc_tol: the error (cells) counted as "within".
    model: "iso" (the four-term fit of a round plume; min_samples None = 5) or "aniso" (the six-term fit of source_aniso.py:
    both widths and the axis angle; min_samples None = 8, never below 6).  The dict carries `model` only where it is "aniso"."""
    if model not in ("iso", "aniso"):
        raise ValueError(f"model={model!r}: \"iso\" or \"aniso\"")
    least = 4 if model == "iso" else 6
    if min_samples is None:
        min_samples = 5 if model == "iso" else 8
    if not isinstance(use_tke, (bool, np.bool_)):
        raise ValueError(f"use_tke={use_tke!r}: True or False")
    if not (isinstance(min_samples, (int, np.integer)) and not isinstance(min_samples, bool) and least <= min_samples < 1 << 31):
        raise ValueError(f"min_samples={min_samples!r}: at least {least} records (the fit has {'four' if least == 4 else 'six'} parameters)")
    if not (_num(background) and np.isfinite(background)):
        raise ValueError(f"background={background!r}: a finite concentration")
    if not (_num(floor) and np.isfinite(floor) and floor >= 0.0):
        raise ValueError(f"floor={floor!r}: a finite, non-negative concentration")
    if not (_num(min_pivot) and np.isfinite(min_pivot) and min_pivot > 0.0):
        raise ValueError(f"min_pivot={min_pivot!r}: a finite positive pivot")
    if not (_num(loc_tol) and loc_tol == loc_tol and loc_tol >= 0.0):
        raise ValueError(f"loc_tol={loc_tol!r}: a non-negative distance in cells")
    cfg = dict(use_tke=bool(use_tke), min_samples=int(min_samples), background=float(background), floor=float(floor),
               min_pivot=float(min_pivot), loc_tol=float(loc_tol))
    if model != "iso":
        cfg["model"] = model
    return cfg


def is_aniso(cfg):
    """Whether a check_source_fit dict (or None) asks for the six-term model."""
    return cfg is not None and cfg.get("model", "iso") == "aniso"


def option(source_fit):
    """The `source_fit=` option of evaluate / ModelEvaluator / EvalTracker: None or False -> None (off), True -> the defaults, a dict
    -> check_source_fit(**dict)."""
    if source_fit is None or source_fit is False:
        return None
    if source_fit is True:
        return check_source_fit()
    if isinstance(source_fit, dict):
        try:
            return check_source_fit(**source_fit)
        except TypeError as e:
            raise ValueError(f"source_fit={source_fit!r}: {e}") from None
    raise ValueError(f"source_fit={source_fit!r}: None, True or a dict of check_source_fit's keywords")


def variant_truth(variant):
    """(sigma, peak) of the procedural plume of an env variant (env.hip: 15 cells for v2.1, 500 / 16 otherwise; peak 100)."""
    return (15.0 if str(variant) == "v2.1" else 500.0 / 16.0), 100.0


# ------------------------------------------------------------------------------------------ the numpy definitions
def fresh_state(n):
    """state f64 [n, 20] of an evaluation that has not stepped yet: all zeros."""
    return np.zeros((n, STATE_N), np.float64)


def _tree(v):
    """wave_sum's tree over axis -2 (64 lanes -> lane 0): lane l += lane l + 32, 16, ... 1."""
    v = v.copy()
    o = 32
    while o > 0:
        v[..., :o, :] = v[..., :o, :] + v[..., o:2 * o, :]
        o >>= 1
    return v[..., 0, :]


def _block256(v):
    w = _tree(v.reshape(4, 64, v.shape[-1]))
    return ((w[0] + w[1]) + w[2]) + w[3]


def cells(pos):
    """i32 cells of f32 positions: min(max((int)v, 0), 499), clamped as a float first (a NaN is cell 0)."""
    return np.fmin(np.fmax(np.asarray(pos, np.float32), np.float32(0.0)), np.float32(499.0)).astype(np.int32)


def used_records(flags, obs, pos, ended=None, use_tke=True, background=0.0, floor=1.0, **_):
    """(used bool [n, k], b f64 [n, k], cell i32 [n, k, 2]) of one chunk: which records uav_source_moments adds.  Records are taken
    up to and including the env's first with bit0 or bit3, never one with bit2, none of an env that comes in ended."""
    flags = np.asarray(flags, np.uint8)
    obs = np.asarray(obs, np.float32)
    n, k = flags.shape
    skip = (flags & 4) != 0
    end = ~skip & ((flags & 9) != 0)
    first = np.where(end.any(1), end.argmax(1), k - 1)
    take = ~skip & (np.arange(k)[None, :] <= first[:, None])
    if ended is not None:
        take &= (np.asarray(ended) == 0)[:, None]
    o2 = obs[:, :, 2]
    if use_tke:
        b = 100.0 * o2.astype(np.float64) - 9.0 * obs[:, :, 3].astype(np.float64)
    else:
        b = 100.0 * o2.astype(np.float64) - np.float64(background)
    with np.errstate(invalid="ignore"):
        used = take & (b > np.float64(floor)) & (o2 < np.float32(1.0))
    return used, b, cells(pos)


def moments_chunk(flags, obs, pos, state, ended=None, use_tke=True, background=0.0, floor=1.0, **_):
    """uav_source_moments: the new state f64 [n, 20] after one chunk of records flags u8 [n, k], obs f32 [n, k, D], pos f32
    [n, k, 2].  THE ORDER OF SUMMATION: lane l of 64 adds the used records i = l (mod 64) in increasing i from zero, the 64 partials
    are added by _tree, the state adds the total."""
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
    r = p * p + q * q
    bu = np.where(used, b, 1.0)
    w, lb = bu * bu, np.log(bu)
    wp, wq, wr = w * p, w * q, w * r
    c = np.stack([np.ones_like(w), w, wp, wq, wr, wp * p, wp * q, wp * r, wq * q, wq * r, wr * r, w * lb, wp * lb, wq * lb, wr * lb], 2)
    c = np.where(used[:, :, None], c, 0.0)
    nb = (k + 63) // 64
    c = np.concatenate([c, np.zeros((n, nb * 64 - k, 15))], 1).reshape(n, nb, 64, 15)
    acc = np.zeros((n, 64, 15), np.float64)
    for blk in range(nb):
        acc = acc + c[:, blk]
    tot = _tree(acc)
    st[live, 0] = st[live, 0] + tot[live, 0]
    st[live, 3:17] = st[live, 3:17] + tot[live, 1:]
    im = np.where(used, b, -np.inf).argmax(1)                   # the first of equal largest
    bm = b[e, im]
    with np.errstate(invalid="ignore"):
        up = live & any_used & (bm > st[:, 17])                 # strictly: an earlier chunk's record wins a tie
    st[up, 17] = bm[up]
    st[up, 18] = cell[e, im, 0][up].astype(np.float64)
    st[up, 19] = cell[e, im, 1][up].astype(np.float64)
    return st


def scaled_system(state):
    """(S f64 [n, 4, 4], h f64 [n, 4], d f64 [n, 4]): A scaled by d_j = sqrt(A_jj) and g / d, the system solve factors."""
    st = np.asarray(state, np.float64).reshape(-1, STATE_N)
    A = np.stack([np.stack([st[:, 3 + _IDX[i][j]] for j in range(4)], 1) for i in range(4)], 1)
    with np.errstate(all="ignore"):
        d = np.sqrt(np.stack([A[:, j, j] for j in range(4)], 1))
        S = A / (d[:, :, None] * d[:, None, :])
        h = st[:, 13:17] / d
    return S, h, d


def coefficients(state, min_pivot=1e-6):
    """(a f64 [n, 4], degenerate bool [n]): the scaled Cholesky by columns, the two triangular solves and the unscaling, in the
    kernel's order of operations (every t = t - L * z one after the other, no fused multiply-add)."""
    S, h, d = scaled_system(state)
    n = S.shape[0]
    L = np.zeros((n, 4, 4), np.float64)
    bad = np.zeros(n, bool)
    with np.errstate(all="ignore"):
        for j in range(4):
            s = S[:, j, j]
            for c in range(j):
                s = s - L[:, j, c] * L[:, j, c]
            bad |= ~(np.isfinite(s) & (s >= np.float64(min_pivot)))
            L[:, j, j] = np.sqrt(s)
            for i in range(j + 1, 4):
                t = S[:, i, j]
                for c in range(j):
                    t = t - L[:, i, c] * L[:, j, c]
                L[:, i, j] = t / L[:, j, j]
        z = np.zeros((n, 4), np.float64)
        u = np.zeros((n, 4), np.float64)
        for j in range(4):
            t = h[:, j]
            for c in range(j):
                t = t - L[:, j, c] * z[:, c]
            z[:, j] = t / L[:, j, j]
        for j in (3, 2, 1, 0):
            t = z[:, j]
            for c in range(j + 1, 4):
                t = t - L[:, c, j] * u[:, c]
            u[:, j] = t / L[:, j, j]
        a = u / d
    return a, bad


def solve(state, min_samples=5, min_pivot=1e-6, **_):
    """uav_source_solve: (est f64 [n, 8], status u8 [n]).  est = {mu_x, mu_y, sigma, peak, strength, largest sample's x, y, b}; the
    first five are NaN unless status is FITTED, all eight for a count of 0."""
    st = np.asarray(state, np.float64).reshape(-1, STATE_N)
    n = st.shape[0]
    est = np.full((n, EST_N), np.nan)
    status = np.zeros(n, np.uint8)
    count = st[:, 0]
    some = count > 0.0
    est[some, 5], est[some, 6], est[some, 7] = st[some, 18], st[some, 19], st[some, 17]
    few = ~(count >= np.float64(min_samples))
    a, bad = coefficients(st, min_pivot)
    with np.errstate(all="ignore"):
        s2 = -1.0 / (2.0 * a[:, 3])
        peaked = np.isfinite(a).all(1) & (a[:, 3] < 0.0) & np.isfinite(s2)
        sigma = SCALE * np.sqrt(s2)
        peak = np.exp(a[:, 0] + (a[:, 1] * a[:, 1] + a[:, 2] * a[:, 2]) * s2 / 2.0)
        mx = st[:, 1] + SCALE * a[:, 1] * s2
        my = st[:, 2] + SCALE * a[:, 2] * s2
        strength = TWO_PI * (sigma * sigma) * peak
    status[:] = np.where(few, FEW, np.where(bad, DEGENERATE, np.where(peaked, FITTED, NOT_A_PEAK)))
    ok = status == FITTED
    for j, v in enumerate((mx, my, sigma, peak, strength)):
        est[ok, j] = v[ok]
    return est, status


def summarise(est, status, src, sigma_true, peak_true, loc_tol):
    """uav_source_summary: dict(sums f64 [12], loc_err f64 [n]).  sums = {envs, fitted, few, degenerate, not a peak, sum of the
    fitted envs' errors, of their squares, how many within loc_tol, sum of |sigma - sigma_true| / sigma_true, of |peak - peak_true|
    / peak_true (each 0 where the truth is not finite and positive), sum of the largest samples' distances to the source, how many
    envs have one}, in summarise's (eval_track.py) order of summation."""
    est, status = np.asarray(est, np.float64).reshape(-1, EST_N), np.asarray(status, np.uint8)
    src = np.asarray(src, np.float64)
    n = status.shape[0]
    fit = status == FITTED
    with np.errstate(invalid="ignore"):
        dx, dy = est[:, 0] - src[:, 0], est[:, 1] - src[:, 1]
        err = np.where(fit, np.sqrt(dx * dx + dy * dy), np.nan)
        within = fit & (err <= np.float64(loc_tol))
        sig_known = bool(np.isfinite(sigma_true) and sigma_true > 0.0)
        peak_known = bool(np.isfinite(peak_true) and peak_true > 0.0)
        sr = np.abs(est[:, 2] - np.float64(sigma_true)) / np.float64(sigma_true) if sig_known else np.zeros(n)
        pr = np.abs(est[:, 3] - np.float64(peak_true)) / np.float64(peak_true) if peak_known else np.zeros(n)
        has = est[:, 7] == est[:, 7]
        mx, my = est[:, 5] - src[:, 0], est[:, 6] - src[:, 1]
        md = np.sqrt(mx * mx + my * my)
    z = np.zeros(n)
    vals = np.stack([fit.astype(np.float64), (status == FEW).astype(np.float64), (status == DEGENERATE).astype(np.float64),
                     (status == NOT_A_PEAK).astype(np.float64), np.where(fit, err, z), np.where(fit, err * err, z),
                     within.astype(np.float64), np.where(fit, sr, z), np.where(fit, pr, z), np.where(has, md, z),
                     has.astype(np.float64)], axis=1)
    acc = np.zeros((SLOTS, SUM_N - 1), np.float64)
    for r0 in range(0, n, SLOTS):
        c = vals[r0:r0 + SLOTS]
        acc[:c.shape[0]] += c
    return {"sums": np.concatenate([[np.float64(n)], _block256(acc)]), "loc_err": err}


def fit_records(chunks, n, ended_of=None, **cfg):
    """The statement over a whole episode: chunks = [(flags, obs, pos)] in time order, each chunk's `ended` taken from
    eval_track.reduce_chunk's state before it (or from ended_of(i) when given) -> (state, est, status)."""
    from .eval_track import fresh_episodes, reduce_chunk
    cfg = check_source_fit(**cfg)
    st, ep, t0 = fresh_state(n), fresh_episodes(n), 0
    for i, (flags, obs, pos) in enumerate(chunks):
        ended = ep[1] if ended_of is None else ended_of(i)
        st = moments_chunk(flags, obs, pos, st, ended, **cfg)
        ep = reduce_chunk(flags, obs, pos, t0, *ep)
        t0 += np.asarray(flags).shape[1]
    est, status = solve(st, **cfg)
    return st, est, status


def source_row(sums):
    """The six eval_curve.csv columns (SOURCE_COLUMNS) from the twelve sums: plain python numbers, NaN where nothing was fitted."""
    S = np.asarray(sums, np.float64)
    n, fit, has = float(S[0]), float(S[1]), float(S[11])
    nan = float("nan")
    return [fit / n if n > 0 else nan, float(S[5]) / fit if fit > 0 else nan, float(S[7]) / fit if fit > 0 else nan,
            float(S[8]) / fit if fit > 0 else nan, float(S[9]) / fit if fit > 0 else nan, float(S[10]) / has if has > 0 else nan]


def metrics(est, status, loc_err):
    """evaluate()'s source_* entries from numpy est [N, 8], status [N], loc_err [N]."""
    est = np.asarray(est, np.float64)
    return {"source_estimate": est[:, 0:2].copy(), "source_sigma": est[:, 2].copy(), "source_peak": est[:, 3].copy(),
            "source_strength": est[:, 4].copy(), "source_status": np.asarray(status, np.uint8).copy(),
            "source_error": np.asarray(loc_err, np.float64).copy(), "source_max_sample": est[:, 5:8].copy()}


def write_estimates(path, m):
    """source_estimates.csv (ESTIMATE_COLUMNS) from evaluate()'s metrics: one row per episode, NaN written as "nan".  The six-term
    model's metrics (source_sigma_minor, source_theta) put Sigma_Minor and Theta behind Sigma, for that model only."""
    import csv
    from .ops import SRC_STATUS_NAMES
    six = "source_sigma_minor" in m
    with open(path, "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        at = ESTIMATE_COLUMNS.index("Sigma") + 1
        w.writerow(ESTIMATE_COLUMNS[:at] + ["Sigma_Minor", "Theta"] + ESTIMATE_COLUMNS[at:] if six else ESTIMATE_COLUMNS)
        for i in range(len(m["source_status"])):
            more = [float(m["source_sigma_minor"][i]), float(m["source_theta"][i])] if six else []
            w.writerow([i + 1, SRC_STATUS_NAMES[int(m["source_status"][i])], *(float(v) for v in m["source_estimate"][i]),
                        float(m["source_sigma"][i]), *more, float(m["source_peak"][i]), float(m["source_strength"][i]),
                        float(m["source_error"][i]), *(float(v) for v in m["source_max_sample"][i])])


# ------------------------------------------------------------------------------------------ the device side
class SourceFit:
    """The estimator's device state for n envs: restart(), chunk(recs, ended) once per chunk of greedy records BEFORE that chunk's
    uav_greedy_reduce, finish(src, ...) after the last.  Launches only: nothing is read by the host."""

    def __init__(self, n, device="cuda", **cfg):
        import torch
        from . import ops
        self.cfg = check_source_fit(**cfg)
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
        ops.source_moments(recs, self._c, self.state, ended)

    def finish(self, src, sigma_true=float("nan"), peak_true=float("nan"), loc_tol=None, sums=None):
        """uav_source_solve, then uav_source_summary against src f64 [n, 2] into `sums` (default: self.sums); returns it."""
        from . import ops
        ops.source_solve(self.state, self._c, self.est, self.status)
        return ops.source_summary(self.est, self.status, src, sigma_true, peak_true, self.cfg["loc_tol"] if loc_tol is None else loc_tol,
                                  self.sums if sums is None else sums, loc_err=self.loc_err)

    def metrics(self):
        """evaluate()'s source_* entries as numpy arrays.  Waits for the device."""
        return metrics(self.est.cpu().numpy(), self.status.cpu().numpy(), self.loc_err.cpu().numpy())
