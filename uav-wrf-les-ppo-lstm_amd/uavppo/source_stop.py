"""The source estimator as a stop rule (evaluate(source_stop=...), EvalTracker(source_stop=...)): the UAV re-fits the source after
every record (source_fit.py's closed form) and stops once the fit has settled and it stands near the fitted source.  No trained
predictor is involved, unlike the ThresholdController and the PeakAndStopPredictor.

THE RULE, for one env.  Records are eligible as source_fit.used_records takes them: up to and including the env's first with bit0
or bit3, never one with bit2, none of an env that comes in ended or already hit; a record that is not eligible changes nothing.
After eligible record i, E_i = source_fit.solve on the moments of the episode's used records 0 .. i.  The record is settled iff E_i
and the previous eligible record's estimate are both FITTED and (mu_i - mu_prev)^2 summed over x and y <= settle_tol^2 (f64, no
square root); run_i counts the settled eligible records ending at i and carries over blocks and chunks.  The rule hits at i iff
run_i >= patience, E_i is FITTED, |f64(pos_i) - mu_i|^2 <= near^2 and t0 + i + 1 >= min_steps.  The first hit ends the episode.

One kernel, uav_source_stop_scan (csrc/source_fit.hip): one wave per env, per block of 64 records (aligned to the chunk's start)
an inclusive Hillis-Steele scan of the 15 contributions, prefix = carry + scan, one solve per eligible lane.  stop_scan_chunk
states it in numpy in that order of operations; stop_rule is the rule alone on given per-record estimates: comparisons and f64
multiply-add only, so it is bit-exact on any input.  With `mark` the kernel writes the hit into the records' flags (bit3 on the
hit, bit2 behind it), after which uav_source_moments, uav_greedy_reduce and uav_greedy_summary see the episode end there.

An evaluation env whose own success radius is large ends its episodes before the rule can: set the radius small (eval_radius)
where the rule is to do the stopping.  What is NOT in here: the rule together with the learned controllers, the step-wise route,
ModelEvaluator (its rule is inside its kernel), anisotropic plumes.
"""
from __future__ import annotations

import numpy as np

from . import source_fit as sf

STATE_N = 27                                 # ops.SRC_STOP_STATE_N
PREV_X, PREV_Y, PREV_FITTED, RUN, HIT_STEP, EST = 17, 18, 19, 20, 21, 22
RULE = slice(PREV_X, EST + 2)                # stop_rule's state: prev mu (2), prev fitted, run, hit step, mu at the hit (2)
NOT_ELIGIBLE = 255
STOP_COLUMN = "Stop_Rate"


def check_source_stop(settle_tol=0.5, patience=3, near=None, min_steps=0):
    """The rule's keywords, refused with the reason (ValueError); returns them as a dict of plain values (near=None -> inf: the
    rule fires wherever the UAV stands).  Pure host arithmetic."""
    if not (sf._num(settle_tol) and np.isfinite(settle_tol) and settle_tol >= 0.0):
        raise ValueError(f"settle_tol={settle_tol!r}: a finite, non-negative distance in cells")
    if not (isinstance(patience, (int, np.integer)) and not isinstance(patience, bool) and 1 <= patience < 1 << 31):
        raise ValueError(f"patience={patience!r}: at least 1 settled record")
    if near is not None and not (sf._num(near) and near == near and near >= 0.0):
        raise ValueError(f"near={near!r}: a non-negative distance in cells, or None (anywhere)")
    if not (isinstance(min_steps, (int, np.integer)) and not isinstance(min_steps, bool) and 0 <= min_steps < 1 << 31):
        raise ValueError(f"min_steps={min_steps!r}: a non-negative number of steps")
    return dict(settle_tol=float(settle_tol), patience=int(patience), near=float("inf") if near is None else float(near),
                min_steps=int(min_steps))


def option(source_stop):
    """The `source_stop=` option of evaluate / EvalTracker: None or False -> None (off), True -> the defaults, a dict ->
    check_source_stop(**dict)."""
    if source_stop is None or source_stop is False:
        return None
    if source_stop is True:
        return check_source_stop()
    if isinstance(source_stop, dict):
        try:
            return check_source_stop(**source_stop)
        except TypeError as e:
            raise ValueError(f"source_stop={source_stop!r}: {e}") from None
    raise ValueError(f"source_stop={source_stop!r}: None, True or a dict of check_source_stop's keywords")


# ------------------------------------------------------------------------------------------ the numpy definitions
def fresh_state(n):
    """state f64 [n, 27] of an evaluation that has not stepped yet: all zeros."""
    return np.zeros((n, STATE_N), np.float64)


def eligible_records(flags, ended=None, state=None):
    """bool [n, k]: the records the rule sees -- up to and including the env's first with bit0 or bit3, never one with bit2, none of
    an env that comes in ended or (state given) already hit."""
    flags = np.asarray(flags, np.uint8)
    n, k = flags.shape
    skip = (flags & 4) != 0
    end = ~skip & ((flags & 9) != 0)
    first = np.where(end.any(1), end.argmax(1), k - 1)
    take = ~skip & (np.arange(k)[None, :] <= first[:, None])
    if ended is not None:
        take &= (np.asarray(ended) == 0)[:, None]
    if state is not None:
        take &= ~(np.asarray(state, np.float64).reshape(n, -1)[:, HIT_STEP] > 0.0)[:, None]
    return take


def _scan64(c):
    """The inclusive Hillis-Steele scan over axis 1 (64 lanes): offsets 1, 2, 4, 8, 16, 32, lane l adds lane l - o's old value."""
    s = c.copy()
    o = 1
    while o < 64:
        s[:, o:] = s[:, o:] + s[:, :-o]
        o <<= 1
    return s


def stop_rule(mu_steps, status_steps, pos, t0, rule_state, cfg):
    """The rule alone on per-record estimates mu_steps f64 [n, k, 2], status_steps u8 [n, k] (255: not eligible), pos f32 [n, k, 2]
    after t0 earlier steps, from rule_state f64 [n, 7] = {previous mu_x, mu_y (0 unless fitted), its fitted bit, run, hit step (0:
    none), mu at the hit} -> (first_hit i32 [n] (-1: none), the new rule_state).  An env whose state holds a hit step is left alone.
    Comparisons and f64 multiply-add only."""
    mu, status = np.asarray(mu_steps, np.float64), np.asarray(status_steps, np.uint8)
    pos = np.asarray(pos, np.float32).astype(np.float64)
    n, k = status.shape
    rs = np.array(rule_state, np.float64).reshape(n, 7).copy()
    tol2, near2 = np.float64(cfg["settle_tol"]) * np.float64(cfg["settle_tol"]), np.float64(cfg["near"]) * np.float64(cfg["near"])
    first_hit = np.full(n, -1, np.int32)
    over = rs[:, 4] > 0.0
    for i in range(k):
        elig = ~over & (status[:, i] != NOT_ELIGIBLE)
        fit = elig & (status[:, i] == sf.FITTED)
        mx, my = np.where(fit, mu[:, i, 0], 0.0), np.where(fit, mu[:, i, 1], 0.0)
        dx, dy = mx - rs[:, 0], my - rs[:, 1]
        settled = fit & (rs[:, 2] != 0.0) & (dx * dx + dy * dy <= tol2)
        run = np.where(elig, np.where(settled, rs[:, 3] + 1.0, 0.0), rs[:, 3])
        with np.errstate(invalid="ignore"):
            nx, ny = pos[:, i, 0] - mx, pos[:, i, 1] - my
            hit = fit & (run >= cfg["patience"]) & (nx * nx + ny * ny <= near2) & (t0 + i + 1 >= cfg["min_steps"])
        rs[:, 0], rs[:, 1] = np.where(elig, mx, rs[:, 0]), np.where(elig, my, rs[:, 1])
        rs[:, 2] = np.where(elig, fit.astype(np.float64), rs[:, 2])
        rs[:, 3] = run
        rs[hit, 4] = np.float64(t0 + i + 1)
        rs[hit, 5], rs[hit, 6] = mx[hit], my[hit]
        first_hit[hit] = i
        over |= hit
    return first_hit, rs


def mark_flags(flags, first_hit):
    """The flags as the kernel rewrites them with mark: bit3 on the hit record, bit2 on every record behind it in the chunk."""
    out = np.array(flags, np.uint8).copy()
    k = out.shape[1]
    for e in np.nonzero(np.asarray(first_hit) >= 0)[0]:
        h = int(first_hit[e])
        out[e, h] |= 8
        out[e, h + 1:k] |= 4
    return out


def stop_scan_chunk(flags, obs, pos, t0, state, ended, fit_cfg, stop_cfg):
    """uav_source_stop_scan: dict(state f64 [n, 27], first_hit i32 [n], mu_steps f64 [n, k, 2], status_steps u8 [n, k], flags (as
    marked), est f64 [n, k, 5] (every eligible record's mu, sigma, peak, strength), systems f64 [n, k, 20] (what each record's
    solve was given, in source_fit's state layout)) after one chunk of records.  THE ORDER OF
    SUMMATION: per block of 64 records from the chunk's start _scan64 over the 15 contributions, prefix = carry + scan, and the
    carry into the next block is the prefix at the block's last eligible lane (the state's accumulators for the first block)."""
    flags = np.asarray(flags, np.uint8)
    n, k = flags.shape
    st = np.array(state, np.float64).reshape(n, STATE_N).copy()
    idle = st[:, HIT_STEP] > 0.0
    if ended is not None:
        idle = idle | (np.asarray(ended) != 0)
    take = eligible_records(flags, idle.astype(np.uint8))
    used, b, cell = sf.used_records(flags, obs, pos, idle.astype(np.uint8), fit_cfg["use_tke"], fit_cfg["background"], fit_cfg["floor"])
    e = np.arange(n)
    c = sf.contributions(used, b, cell, st)                     # fixes the centre of an env without one, in st
    nb = (k + 63) // 64
    c = np.concatenate([c, np.zeros((n, nb * 64 - k, 15))], 1)
    tk = np.concatenate([take, np.zeros((n, nb * 64 - k), bool)], 1)
    carry = np.concatenate([st[:, 0:1], st[:, 3:17]], 1)
    prefix = np.zeros((n, nb * 64, 15), np.float64)
    for blk in range(nb):
        s = slice(blk * 64, blk * 64 + 64)
        prefix[:, s] = carry[:, None, :] + _scan64(c[:, s])
        has = tk[:, s].any(1)
        le = 63 - tk[:, s][:, ::-1].argmax(1)
        carry = np.where(has[:, None], prefix[e, blk * 64 + le], carry)
    prefix = prefix[:, :k]
    sys = np.zeros((n, k, sf.STATE_N), np.float64)               # one system per record, in source_fit's state layout
    sys[:, :, 0] = prefix[:, :, 0]
    sys[:, :, 1:3] = st[:, None, 1:3]
    sys[:, :, 3:17] = prefix[:, :, 1:]
    est, status = sf.solve(sys.reshape(n * k, sf.STATE_N), fit_cfg["min_samples"], fit_cfg["min_pivot"])
    est, status = est.reshape(n, k, sf.EST_N)[:, :, :5], status.reshape(n, k)
    status = np.where(take, status, NOT_ELIGIBLE).astype(np.uint8)
    mu = np.where((status == sf.FITTED)[:, :, None], est[:, :, :2], np.nan)
    first_hit, rs = stop_rule(mu, status, pos, t0, st[:, RULE], stop_cfg)
    hit = first_hit >= 0
    behind = np.arange(k)[None, :] > np.where(hit, first_hit, k)[:, None]
    status = np.where(behind, NOT_ELIGIBLE, status).astype(np.uint8)
    mu = np.where(behind[:, :, None], np.nan, mu)
    seen = take & ~behind
    has = seen.any(1)
    at = k - 1 - seen[:, ::-1].argmax(1)                        # the hit, else the chunk's last eligible record
    st[has, 0] = prefix[e, at, 0][has]
    st[has, 3:17] = prefix[e, at, 1:][has]
    st[~has, 1:3] = np.array(state, np.float64).reshape(n, STATE_N)[~has, 1:3]
    st[:, RULE] = rs
    st[hit, EST:EST + 5] = est[e, at][hit]
    return {"state": st, "first_hit": first_hit, "mu_steps": mu, "status_steps": status, "flags": mark_flags(flags, first_hit),
            "est": est, "systems": sys}


def stop_records(chunks, n, fit_cfg, stop_cfg, ended_of=None):
    """The statement over a whole episode: chunks = [(flags, obs, pos)] in time order -> dict(state, stop_step i64 [n] (0: the rule
    did not fire), flags (each chunk's, as marked), ep (eval_track.reduce_chunk's state over the marked flags), fit (source_fit's
    (state, est, status) over them)): what evaluate(source_stop=...) computes from the same records."""
    from .eval_track import fresh_episodes, reduce_chunk
    st, fit, ep, t0, marked = fresh_state(n), sf.fresh_state(n), fresh_episodes(n), 0, []
    for i, (flags, obs, pos) in enumerate(chunks):
        ended = ep[1] if ended_of is None else ended_of(i)
        out = stop_scan_chunk(flags, obs, pos, t0, st, ended, fit_cfg, stop_cfg)
        st = out["state"]
        marked.append(out["flags"])
        fit = sf.moments_chunk(out["flags"], obs, pos, fit, ended, **fit_cfg)
        ep = reduce_chunk(out["flags"], obs, pos, t0, *ep)
        t0 += np.asarray(flags).shape[1]
    est, status = sf.solve(fit, **fit_cfg)
    return {"state": st, "stop_step": st[:, HIT_STEP].astype(np.int64), "flags": marked, "ep": ep, "fit": (fit, est, status)}


# ------------------------------------------------------------------------------------------ the device side
class SourceStop:
    """The rule's device state for n envs: restart(), scan(recs, t0, ended, active) once per chunk of greedy records BEFORE that
    chunk's uav_source_moments / uav_greedy_reduce (it marks the records' flags).  Launches only: nothing is read by the host."""

    def __init__(self, n, device="cuda", fit_cfg=None, **cfg):
        import torch
        from . import ops
        self.fit_cfg = sf.check_source_fit(**(fit_cfg or {}))
        if sf.is_aniso(self.fit_cfg):
            raise ValueError("source_stop: not with source_fit model \"aniso\": the scan solves the four-term system per record")
        self.cfg = check_source_stop(**cfg)
        self.n, self.device = int(n), torch.device(device)
        self._f, self._s = ops.source_fit_cfg(**self.fit_cfg), ops.source_stop_cfg(**self.cfg)
        self.state = torch.zeros(self.n, STATE_N, dtype=torch.float64, device=self.device)
        self.first_hit = torch.zeros(self.n, dtype=torch.int32, device=self.device)

    def restart(self):
        self.state.zero_()

    def scan(self, recs, t0, ended=None, active=None, mu_steps=None, status_steps=None, mark=True):
        """ended u8 [n] or None: envs whose episodes ended earlier; active u8 [n] or None: cleared at the hits.  Returns first_hit
        i32 [n], the chunk's record of each env's hit or -1 (overwritten by the next scan)."""
        from . import ops
        return ops.source_stop_scan(recs, t0, self._f, self._s, self.state, self.first_hit, ended, active, mu_steps, status_steps, mark)

    def stop_steps(self):
        """i64 [n] on the device: the step each env's rule fired at, 0 where it did not."""
        import torch
        return self.state[:, HIT_STEP].to(torch.int64)
