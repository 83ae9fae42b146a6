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
are tested against bit for bit.  They are written once for any basis (ISO here, ANISO for source_aniso.py's six-term model), as
csrc/source_core.h and csrc/source_solve.h are.  Estimates during the episode, and the estimator as a stop rule, are in source_stop.py
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
class Basis:
    """One model of ln b: n_phi basis functions phi(p, q) -> list, the state layout derived from n_phi (csrc/source_solve.h
    SourceLayout: count, cx, cy | A, the upper triangle by rows | g | the largest b, its x, its y), the widths of est and sums, the
    default min_samples and closed_form(a, cx, cy) -> (the fitted values in est's order, which systems are a peak)."""

    def __init__(self, n_phi, est_n, sum_n, min_samples, phi, closed_form):
        self.n_phi, self.est_n, self.sum_n, self.min_samples, self.phi, self.closed_form = n_phi, est_n, sum_n, min_samples, phi, closed_form
        self.n_a = n_phi * (n_phi + 1) // 2
        self.n_acc, self.st_a, self.st_g, self.st_bmax = 1 + self.n_a + n_phi, 3, 3 + self.n_a, 3 + self.n_a + n_phi
        self.state_n, self.fit_n = self.st_bmax + 3, est_n - 3
        tri = [(i, j) for i in range(n_phi) for j in range(i, n_phi)]
        self.idx = [[tri.index((min(i, j), max(i, j))) for j in range(n_phi)] for i in range(n_phi)]


def _closed_form_iso(a, cx, cy):
    s2 = -1.0 / (2.0 * a[:, 3])
    peaked = np.isfinite(a).all(1) & (a[:, 3] < 0.0) & np.isfinite(s2)
    sigma = SCALE * np.sqrt(s2)
    peak = np.exp(a[:, 0] + (a[:, 1] * a[:, 1] + a[:, 2] * a[:, 2]) * s2 / 2.0)
    return (cx + SCALE * a[:, 1] * s2, cy + SCALE * a[:, 2] * s2, sigma, peak, TWO_PI * (sigma * sigma) * peak), peaked


def _closed_form_aniso(a, cx, cy):
    from .source_aniso import closed_form6
    return closed_form6(a, cx, cy)


ISO = Basis(4, EST_N, SUM_N, 5, lambda p, q: [np.ones_like(p), p, q, p * p + q * q], _closed_form_iso)
ANISO = Basis(6, 10, 16, 8, lambda p, q: [np.ones_like(p), p, q, p * p, p * q, q * q], _closed_form_aniso)
assert ISO.state_n == STATE_N and ISO.idx == [list(r) for r in _IDX]


def basis_of(cfg):
    """ISO or ANISO of a check_source_fit dict (or keywords with `model`)."""
    return ANISO if is_aniso(cfg) else ISO


def fresh_state(n, basis=ISO):
    """state f64 [n, 20] (33 for ANISO) of an evaluation that has not stepped yet: all zeros."""
    return np.zeros((n, basis.state_n), np.float64)


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


def contributions(used, b, cell, st, basis=ISO):
    """c f64 [n, k, n_acc] of a chunk's records (zero where not used): 1 | (w phi_i) phi_j for i <= j by rows, row 0 being w itself
    and then w phi_j | (w phi_i) ln b, with w = b^2 and p, q the cell's offset from the centre / SCALE.  The centre of an env
    without one (count 0) is fixed first, IN st: the cell of the env's first used record.  The moments and the stop scan add these.
    For ISO (r = p p + q q, wp = w * p, ...): 1 | w, wp, wq, wr, wp * p, wp q, wp r, wq q, wq r, wr r | w lb, wp lb, wq lb, wr lb."""
    e, i0 = np.arange(used.shape[0]), used.argmax(1)
    new_c = used.any(1) & ~(st[:, 0] > 0.0)
    st[new_c, 1] = cell[e, i0, 0][new_c].astype(np.float64)
    st[new_c, 2] = cell[e, i0, 1][new_c].astype(np.float64)
    p = (cell[:, :, 0].astype(np.float64) - st[:, 1:2]) / SCALE
    q = (cell[:, :, 1].astype(np.float64) - st[:, 2:3]) / SCALE
    bu = np.where(used, b, 1.0)
    w, lb = bu * bu, np.log(bu)
    phi = basis.phi(p, q)
    wphi = [w] + [w * f for f in phi[1:]]
    cols = [np.ones_like(w)] + [wphi[i] * phi[j] if j else wphi[i] for i in range(basis.n_phi) for j in range(i, basis.n_phi)]
    cols += [wf * lb for wf in wphi]
    return np.where(used[:, :, None], np.stack(cols, 2), 0.0)


def moments_chunk(flags, obs, pos, state, ended=None, use_tke=True, background=0.0, floor=1.0, basis=ISO, **_):
    """uav_source_moments (uav_source_moments6 for ANISO): the new state f64 [n, state_n] after one chunk of records flags u8 [n, k],
    obs f32 [n, k, D], pos f32 [n, k, 2].  THE ORDER OF SUMMATION: lane l of 64 adds the used records i = l (mod 64) in increasing i
    from zero, the 64 partials are added by _tree, the state adds the total."""
    used, b, cell = used_records(flags, obs, pos, ended, use_tke, background, floor)
    n, k = used.shape
    st = np.array(state, np.float64).reshape(n, basis.state_n).copy()
    live = np.ones(n, bool) if ended is None else np.asarray(ended) == 0
    c = contributions(used, b, cell, st, basis)
    nb = (k + 63) // 64
    c = np.concatenate([c, np.zeros((n, nb * 64 - k, basis.n_acc))], 1).reshape(n, nb, 64, basis.n_acc)
    acc = np.zeros((n, 64, basis.n_acc), np.float64)
    for blk in range(nb):
        acc = acc + c[:, blk]
    tot = _tree(acc)
    A, BM = slice(basis.st_a, basis.st_bmax), basis.st_bmax
    st[live, 0] = st[live, 0] + tot[live, 0]
    st[live, A] = st[live, A] + tot[live, 1:]
    e, im = np.arange(n), np.where(used, b, -np.inf).argmax(1)  # the first of equal largest
    bm = b[e, im]
    with np.errstate(invalid="ignore"):
        up = live & used.any(1) & (bm > st[:, BM])              # strictly: an earlier chunk's record wins a tie
    st[up, BM] = bm[up]
    st[up, BM + 1] = cell[e, im, 0][up].astype(np.float64)
    st[up, BM + 2] = cell[e, im, 1][up].astype(np.float64)
    return st


def scaled_system(state, basis=ISO):
    """(S f64 [n, N, N], h f64 [n, N], d f64 [n, N]): A scaled by d_j = sqrt(A_jj) and g / d, the system solve factors."""
    st, N = np.asarray(state, np.float64).reshape(-1, basis.state_n), basis.n_phi
    A = np.stack([np.stack([st[:, basis.st_a + basis.idx[i][j]] for j in range(N)], 1) for i in range(N)], 1)
    with np.errstate(all="ignore"):
        d = np.sqrt(np.stack([A[:, j, j] for j in range(N)], 1))
        S = A / (d[:, :, None] * d[:, None, :])
        h = st[:, basis.st_g:basis.st_g + N] / d
    return S, h, d


def cholesky(state, min_pivot=1e-6, basis=ISO):
    """(a f64 [n, N], degenerate bool [n], smallest pivot f64 [n]): the scaled Cholesky by columns, the two triangular solves and
    the unscaling, in the kernel's order of operations (csrc/source_solve.h chol_solve: every t = t - L * z one after the other, no
    fused multiply-add)."""
    S, h, d = scaled_system(state, basis)
    n, N = S.shape[0], basis.n_phi
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


def coefficients(state, min_pivot=1e-6, basis=ISO):
    """(a f64 [n, N], degenerate bool [n]) of cholesky."""
    return cholesky(state, min_pivot, basis)[:2]


def solve(state, min_samples=None, min_pivot=1e-6, basis=ISO, **_):
    """uav_source_solve (uav_source_solve6 for ANISO): (est f64 [n, est_n], status u8 [n]).  est = {the basis's fitted values (ISO:
    mu_x, mu_y, sigma, peak, strength), largest sample's x, y, b}; the fitted values are NaN unless status is FITTED, all of est
    for a count of 0.  min_samples None: the basis's default."""
    st = np.asarray(state, np.float64).reshape(-1, basis.state_n)
    n, F, BM = st.shape[0], basis.fit_n, basis.st_bmax
    est = np.full((n, basis.est_n), np.nan)
    status = np.zeros(n, np.uint8)
    count = st[:, 0]
    some = count > 0.0
    est[some, F], est[some, F + 1], est[some, F + 2] = st[some, BM + 1], st[some, BM + 2], st[some, BM]
    few = ~(count >= np.float64(basis.min_samples if min_samples is None else min_samples))
    a, bad = coefficients(st, min_pivot, basis)
    with np.errstate(all="ignore"):
        vals, peaked = basis.closed_form(a, st[:, 1], st[:, 2])
    status[:] = np.where(few, FEW, np.where(bad, DEGENERATE, np.where(peaked, FITTED, NOT_A_PEAK)))
    ok = status == FITTED
    for j, v in enumerate(vals):
        est[ok, j] = v[ok]
    return est, status


def summary_sums(basis, est, status, src, loc_tol, truth_columns):
    """The sums both summary kernels share: dict(sums f64 [sum_n], loc_err f64 [n]).  sums = {envs | fitted, few, degenerate, not a
    peak, the fitted envs' errors, their squares, how many within loc_tol | the model's truth_columns(fit) | the largest samples'
    distances to the source, how many envs have one | what truth_columns gave behind those}.  THE ORDER OF SUMMATION: slot j of
    256 adds the envs j, j + 256, ... one after the other, then _block256 (uav_greedy_summary's order)."""
    est, status = np.asarray(est, np.float64).reshape(-1, basis.est_n), np.asarray(status, np.uint8)
    src = np.asarray(src, np.float64)
    n, F = status.shape[0], basis.fit_n
    fit = status == FITTED
    with np.errstate(all="ignore"):
        dx, dy = est[:, 0] - src[:, 0], est[:, 1] - src[:, 1]
        err = np.where(fit, np.sqrt(dx * dx + dy * dy), np.nan)
        within = fit & (err <= np.float64(loc_tol))
        has = est[:, F + 2] == est[:, F + 2]
        mx, my = est[:, F] - src[:, 0], est[:, F + 1] - src[:, 1]
        md = np.sqrt(mx * mx + my * my)
        middle, last = truth_columns(est, fit)
    z = np.zeros(n)
    vals = np.stack([fit.astype(np.float64), (status == FEW).astype(np.float64), (status == DEGENERATE).astype(np.float64),
                     (status == NOT_A_PEAK).astype(np.float64), np.where(fit, err, z), np.where(fit, err * err, z),
                     within.astype(np.float64), *middle, np.where(has, md, z), has.astype(np.float64), *last], axis=1)
    acc = np.zeros((SLOTS, basis.sum_n - 1), np.float64)
    for r0 in range(0, n, SLOTS):
        c = vals[r0:r0 + SLOTS]
        acc[:c.shape[0]] += c
    return {"sums": np.concatenate([[np.float64(n)], _block256(acc)]), "loc_err": err}


def summarise(est, status, src, sigma_true, peak_true, loc_tol):
    """uav_source_summary: dict(sums f64 [12], loc_err f64 [n]).  sums = {envs, fitted, few, degenerate, not a peak, sum of the
    fitted envs' errors, of their squares, how many within loc_tol, sum of |sigma - sigma_true| / sigma_true, of |peak - peak_true|
    / peak_true (each 0 where the truth is not finite and positive), sum of the largest samples' distances to the source, how many
    envs have one}, in summary_sums' order of summation."""
    def truth_columns(est, fit):
        z = np.zeros(len(fit))
        sig_known = bool(np.isfinite(sigma_true) and sigma_true > 0.0)
        peak_known = bool(np.isfinite(peak_true) and peak_true > 0.0)
        sr = np.abs(est[:, 2] - np.float64(sigma_true)) / np.float64(sigma_true) if sig_known else z
        pr = np.abs(est[:, 3] - np.float64(peak_true)) / np.float64(peak_true) if peak_known else z
        return [np.where(fit, sr, z), np.where(fit, pr, z)], []
    return summary_sums(ISO, est, status, src, loc_tol, truth_columns)


def fit_records(chunks, n, ended_of=None, **cfg):
    """The statement over a whole episode: chunks = [(flags, obs, pos)] in time order, each chunk's `ended` taken from
    eval_track.reduce_chunk's state before it (or from ended_of(i) when given) -> (state, est, status); cfg's model is the basis."""
    from .eval_track import fresh_episodes, reduce_chunk
    cfg = check_source_fit(**cfg)
    basis = basis_of(cfg)
    st, ep, t0 = fresh_state(n, basis), fresh_episodes(n), 0
    for i, (flags, obs, pos) in enumerate(chunks):
        ended = ep[1] if ended_of is None else ended_of(i)
        st = moments_chunk(flags, obs, pos, st, ended, basis=basis, **cfg)
        ep = reduce_chunk(flags, obs, pos, t0, *ep)
        t0 += np.asarray(flags).shape[1]
    est, status = solve(st, basis=basis, **cfg)
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
    uav_greedy_reduce, finish(src, ...) after the last.  cfg's model ("iso" / "aniso") chooses the entry points and the buffer
    widths.  Launches only: nothing is read by the host."""

    def __init__(self, n, device="cuda", **cfg):
        import torch
        from . import ops
        self.cfg = check_source_fit(**cfg)
        self.aniso, b = is_aniso(self.cfg), basis_of(self.cfg)
        self.n, self.device = int(n), torch.device(device)
        self._c = ops.source_fit_cfg(**self.cfg)
        self._moments, self._solve = (ops.source_moments6, ops.source_solve6) if self.aniso else (ops.source_moments, ops.source_solve)
        self.state = torch.zeros(self.n, b.state_n, dtype=torch.float64, device=self.device)
        self.est = torch.zeros(self.n, b.est_n, dtype=torch.float64, device=self.device)
        self.status = torch.zeros(self.n, dtype=torch.uint8, device=self.device)
        self.loc_err = torch.zeros(self.n, dtype=torch.float64, device=self.device)
        self.sums = torch.zeros(b.sum_n, dtype=torch.float64, device=self.device)

    def restart(self):
        self.state.zero_()

    def chunk(self, recs, ended=None):
        """ended u8 [n]: ep_state as it stands before this chunk's uav_greedy_reduce, or None (nothing has ended)."""
        self._moments(recs, self._c, self.state, ended)

    def finish(self, src, sigma_true=float("nan"), peak_true=float("nan"), truth=None, loc_tol=None, sums=None):
        """The model's solve, then its summary against src f64 [n, 2] into `sums` (default: self.sums); returns it.  The truth is
        sigma_true and peak_true for "iso", truth f64 [n, 4] = {sigma_major, sigma_minor, theta, peak} or None for "aniso"."""
        from . import ops
        self._solve(self.state, self._c, self.est, self.status)
        loc_tol, sums = self.cfg["loc_tol"] if loc_tol is None else loc_tol, self.sums if sums is None else sums
        if self.aniso:
            return ops.source_summary6(self.est, self.status, src, truth, loc_tol, sums, loc_err=self.loc_err)
        return ops.source_summary(self.est, self.status, src, sigma_true, peak_true, loc_tol, sums, loc_err=self.loc_err)

    def metrics(self):
        """evaluate()'s source_* entries of the model as numpy arrays.  Waits for the device."""
        from .source_aniso import metrics6
        return (metrics6 if self.aniso else metrics)(self.est.cpu().numpy(), self.status.cpu().numpy(), self.loc_err.cpu().numpy())
