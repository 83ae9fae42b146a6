"""Greedy records for the estimator's stop rule, shared by tests/test_source_stop_host.py and tests/test_gpu_source_stop.py: the
twelve kinds of _source_fit_cases.episodes, and walkers that approach a source axis by axis and then hover over it (E3's formula
restated in numpy, as in _source_fit_cases).  margins() is the condition on the inputs under which the device's decisions must
equal the statement's although its log differs in the last bit."""
import numpy as np

from _source_fit_cases import cells, episodes

NAN = float("nan")
TKE_OFF = dict(use_tke=False, background=2.9, floor=20.0)
# the shapes of the GPU test (n, k, D, seed): every n and k the issue names, D = 6 and 8
SHAPES = [(1, 250, 6, 0), (5, 130, 8, 0), (64, 65, 6, 0), (257, 64, 8, 0), (64, 63, 6, 0), (5, 7, 8, 0), (5, 1, 6, 0), (257, 250, 6, 0)]
SPLITS = (1, 31, 63, 64)


def walkers(n, k, D, seed=0, done_at=None):
    """dict(flags, obs, pos, ended, src, sigma) of n walkers over k steps: env e starts 30 .. 110 cells from its source, moves 7
    cells per step along the axis with the larger distance left (wind noise of 1.5 cells on both), so it overshoots and hovers;
    every fifth env starts 140 cells off and walks away (no usable record: its rule never fires).  done_at: {env: record} gets bit0 | bit1 there and bit2 (NaN obs /
    pos) behind it."""
    rng = np.random.default_rng(7919 * seed + 31 * n + k + D)
    src = rng.uniform(150.0, 350.0, (n, 2))
    sigma = np.where(np.arange(n) % 2 == 0, 15.0, 500.0 / 16.0)
    ang = rng.uniform(0.0, 2.0 * np.pi, n)
    away = np.arange(n) % 5 == 4
    p = src + (np.where(away, 140.0, rng.uniform(30.0, 110.0, n)) * np.array([np.cos(ang), np.sin(ang)])).T
    pos = np.empty((n, k, 2), np.float64)
    for i in range(k):
        d = src - p
        ax = (np.abs(d[:, 1]) > np.abs(d[:, 0])).astype(int)
        step = np.zeros((n, 2))
        step[np.arange(n), ax] = 7.0 * np.sign(d[np.arange(n), ax]) * np.where(away, -1.0, 1.0)
        p = np.clip(p + step + rng.normal(0.0, 1.5, (n, 2)), 1.0, 498.0)
        pos[:, i] = p
    pos = pos.astype(np.float32)
    tke = rng.uniform(0.0, 6.0, (n, k))
    c = cells(pos).astype(np.float64)
    d2 = (c[:, :, 0] - src[:, None, 0]) ** 2 + (c[:, :, 1] - src[:, None, 1]) ** 2
    conc = np.clip(100.0 * np.exp(-d2 / (2.0 * sigma[:, None] ** 2)) + tke, 0.0, 100.0)
    obs = rng.uniform(0.0, 1.0, (n, k, D)).astype(np.float32)
    obs[:, :, 0:2] = pos / np.float32(500.0)
    obs[:, :, 2] = (conc / 100.0).astype(np.float32)
    obs[:, :, 3] = (tke / 9.0).astype(np.float32)
    flags = np.zeros((n, k), np.uint8)
    for e, i in (done_at or {}).items():
        if e < n and i < k:
            flags[e, i] = 3
            flags[e, i + 1:] = 4
            obs[e, i + 1:] = NAN
            pos[e, i + 1:] = NAN
    return {"flags": flags, "obs": obs, "pos": pos, "ended": np.zeros(n, np.uint8), "src": src, "sigma": sigma}


def start_state(ep):
    """state f64 [n, 27] a case set starts from: zeros, and sentinels in the envs that come in ended"""
    n = ep["flags"].shape[0]
    st = np.zeros((n, 27), np.float64)
    gone = ep["ended"] != 0
    st[gone] = 0.5 + np.arange(27 * int(gone.sum()), dtype=np.float64).reshape(-1, 27)
    return st


def case_sets(n, k, D, seed=0):
    """[(name, records, fit cfg keywords)]: the case sets of one shape"""
    return [("twelve kinds", episodes(n, k, D, seed), {}), ("walkers", walkers(n, k, D, seed, {0: 40, 3: 5}), {}),
            ("walkers, constant background", walkers(n, k, D, seed + 1), TKE_OFF)]


# the shapes whose chunk the tests also cut in two at SPLITS
SPLIT_SHAPES = [(65, 130, 6, 1), (257, 65, 8, 1)]


def placed_hits():
    """[(name, records, fit cfg keywords, stop cfg keywords, split or None, the chunk record of the hit in envs that settle
    early)]: hits steered by min_steps onto lane 0 and lane 63 of a block, onto a chunk's first record with the run carried in, and
    onto the very record that is also `done` (env 0 of the walkers: record 40); the last entry has `near` decide (no record named)."""
    w = walkers(20, 130, 6, 3, {0: 40})
    return [("lane 0 of the second block", w, {}, dict(min_steps=65), None, 64), ("lane 63", w, {}, dict(min_steps=64), None, 63),
            ("the chunk's first record, the run carried in", w, {}, dict(min_steps=65), 64, 64),
            ("the record that is also done", w, {}, dict(min_steps=41), None, 40),
            ("near the estimate only, a wider tolerance", w, {}, dict(near=6.0, settle_tol=2.0, patience=5), None, None)]


def drive(ss, ep, fit_cfg, stop_cfg, cuts, scan=None):
    """The statement (or `scan`, a function of its signature) over the pieces cuts[j] .. cuts[j + 1] of a case set's chunk, with
    eval_track.reduce_chunk's ep_state over the marked flags as each piece's `ended` -- as the evaluation drives the kernel.
    Returns (final state, [each piece's output, with its `ended` and the state it started from])."""
    from uavppo import eval_track as et
    n = ep["flags"].shape[0]
    st, eps, outs = start_state(ep), (np.zeros(n, np.int32), ep["ended"].copy(), np.zeros((n, 2))), []
    for a, b in zip(cuts[:-1], cuts[1:]):
        f, o, p = ep["flags"][:, a:b], ep["obs"][:, a:b], ep["pos"][:, a:b]
        out = dict((scan or ss.stop_scan_chunk)(f, o, p, a, st, eps[1], fit_cfg, stop_cfg))
        out["ended"], out["start"], out["t0"] = eps[1], st, a
        eps = et.reduce_chunk(out["flags"], o, p, a, *eps)
        st = out["state"]
        outs.append(out)
    return st, outs


def margins(sf, ss, ep, fit_cfg, stop_cfg, splits=(None,)):
    """Asserts the margin property of one case set for every split of its chunk (None: one piece; a list: the cuts themselves): on every eligible record of the
    statement no move^2 and no near^2 within 1e-6 relative of its threshold, the statuses unchanged under min_pivot (1 +- 1e-6),
    |a3| > 1e-9 wherever the pivots pass, cond(S) <= 1e8 on FITTED records.  Returns how many records were looked at."""
    n, k = ep["flags"].shape
    fit_cfg, stop_cfg = sf.check_source_fit(**fit_cfg), ss.check_source_stop(**stop_cfg)
    cannot = dict(stop_cfg, patience=1 << 30)
    tol2, near2 = stop_cfg["settle_tol"] ** 2, stop_cfg["near"] ** 2
    seen = 0
    for s in splits:
        cuts = list(s) if isinstance(s, (list, tuple)) else [0, k] if s is None or s >= k else [0, s, k]
        prev, pfit = np.zeros((n, 2)), np.zeros(n, bool)
        for out in drive(ss, ep, fit_cfg, cannot, cuts)[1]:
            a, b = out["t0"], out["t0"] + out["flags"].shape[1]
            f, o, p = ep["flags"][:, a:b], ep["obs"][:, a:b], ep["pos"][:, a:b]
            for scale in (1 - 1e-6, 1 + 1e-6):
                other = ss.stop_scan_chunk(f, o, p, a, out["start"], out["ended"], dict(fit_cfg, min_pivot=fit_cfg["min_pivot"] * scale), cannot)
                assert np.array_equal(other["status_steps"], out["status_steps"])
            status, mu = out["status_steps"], out["mu_steps"]
            for i in range(b - a):
                el = status[:, i] != 255
                fit = status[:, i] == 0
                both = fit & pfit
                mv = ((mu[:, i] - prev) ** 2).sum(1)
                assert not (both & (np.abs(mv - tol2) <= 1e-6 * tol2)).any()
                if np.isfinite(near2):
                    nd = ((p[:, i].astype(np.float64) - mu[:, i]) ** 2).sum(1)
                    assert not (fit & (np.abs(nd - near2) <= 1e-6 * near2)).any()
                prev = np.where(el[:, None], np.where(fit[:, None], mu[:, i], 0.0), prev)
                pfit = np.where(el, fit, pfit)
                seen += int(el.sum())
            # the systems behind the estimates: a3 and the conditioning, from the prefixes the statement solved
            sys = out["systems"]
            a3, bad = sf.coefficients(sys.reshape(-1, sf.STATE_N), fit_cfg["min_pivot"])
            a3 = a3[:, 3].reshape(status.shape)
            tried = (status != 255) & (status != 1) & ~bad.reshape(status.shape)
            with np.errstate(invalid="ignore"):
                assert (np.abs(a3[tried]) > 1e-9).all()
            S = sf.scaled_system(sys.reshape(-1, sf.STATE_N))[0][(status == 0).reshape(-1)]
            if len(S):
                assert np.linalg.cond(S).max() <= 1e8
    return seen
