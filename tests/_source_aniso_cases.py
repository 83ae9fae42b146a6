"""Synthetic greedy records on anisotropic plumes, shared by tests/test_source_aniso_host.py and tests/test_gpu_source_aniso.py: the
plume term of uav_plume_bank (uavppo.source_aniso.plume_base) plus a turbulence channel, sampled by walkers around random sources.
obs is f32 as the kernels write it."""
import numpy as np

from _source_fit_cases import cells

NAN = float("nan")
FITTED, FEW, DEGENERATE, NOT_A_PEAK = 0, 1, 2, 3


def _records(pos, field_of, tke, D, rng):
    """obs f32 [n, k, D] of walkers at pos f32 [n, k, 2]: field_of(cell f64 [n, k, 2]) -> the plume term, tke [n, k] on top."""
    c = cells(pos).astype(np.float64)
    conc = np.clip(field_of(c) + tke, 0.0, 100.0)
    n, k = tke.shape
    obs = rng.uniform(0.0, 1.0, (n, k, D)).astype(np.float32)
    obs[:, :, 0:2] = pos / np.float32(500.0)
    obs[:, :, 2] = (conc / 100.0).astype(np.float32)
    obs[:, :, 3] = (tke / 9.0).astype(np.float32)
    return obs


def ellipse_field(src, s_major, s_minor, theta, peak):
    """field_of for _records: each env's own elliptical Gaussian, through source_aniso.plume_base row by row."""
    from uavppo import source_aniso as sa
    params = sa.plume_params(src, s_major, s_minor, theta, peak)

    def field_of(c):
        return np.stack([sa.plume_base(params[e], c[e, :, 0], c[e, :, 1]) for e in range(c.shape[0])])
    return field_of


def clean_walkers(n=400, k=48, D=6, seed=0, ratio=(1.5, 3.0)):
    """The recipe the six-term fit's accuracy is stated for: n episodes of k records, walkers at 0.5 .. 2 sigma in the ellipse's frame
    (any direction), axis ratio U[ratio], major sigma 20 .. 45 cells, sources in 150 .. 350, peak 100, a turbulence channel of 0 .. 6
    that the estimator subtracts.  No episode ends: flags are 0.  dict(flags, obs, pos, src, truth f64 [n, 4] = {sigma_major,
    sigma_minor, theta, peak})."""
    rng = np.random.default_rng(4000037 * seed + 101 * n + k)
    src = rng.uniform(150.0, 350.0, (n, 2))
    s_major = rng.uniform(20.0, 45.0, n)
    s_minor = s_major / rng.uniform(ratio[0], ratio[1], n)
    theta = rng.uniform(0.0, np.pi, n)
    peak = np.full(n, 100.0)
    rad = rng.uniform(0.5, 2.0, (n, k))
    ang = rng.uniform(0.0, 2.0 * np.pi, (n, k))
    u, v = rad * np.cos(ang) * s_major[:, None], rad * np.sin(ang) * s_minor[:, None]
    cs, sn = np.cos(theta)[:, None], np.sin(theta)[:, None]
    pos = (src[:, None, :] + np.stack([u * cs - v * sn, u * sn + v * cs], 2)).astype(np.float32)
    tke = rng.uniform(0.0, 6.0, (n, k))
    obs = _records(pos, ellipse_field(src, s_major, s_minor, theta, peak), tke, D, rng)
    return {"flags": np.zeros((n, k), np.uint8), "obs": obs, "pos": pos, "src": src,
            "truth": np.stack([s_major, s_minor, theta, peak], 1)}


KINDS = ("ends by bit0", "ends by bit3, stepped records of another plume behind it", "ends nowhere", "comes in ended", "straight track",
         "saddle", "bowl", "0 usable records", "5 usable records", "8 usable records", "round plume", "clipped cells")
K = len(KINDS)
# uav_source_solve6's status where the chunk is long enough for the kind to show (k >= MIN_K), min_samples = 8; None: not solved
EXPECTED = (FITTED, FITTED, FITTED, None, DEGENERATE, NOT_A_PEAK, NOT_A_PEAK, FEW, FEW, FITTED, FITTED, FITTED)
MIN_K = 63


def episodes6(n, k, D, seed=0):
    """dict(flags u8 [n, k], obs f32 [n, k, D], pos f32 [n, k, 2], ended u8 [n], state f64 [n, 33] (the start state: zeros, and
    sentinels in the envs that come in ended), src f64 [n, 2], truth f64 [n, 4], kind i64 [n]).  Env e is of kind KINDS[e % 12].
    The obs / pos of every bit2 (not stepped) record are NaN."""
    rng = np.random.default_rng(1000003 * seed + 1009 * n + 17 * k + D)
    e = np.arange(n)
    kind = e % K
    src = rng.uniform(150.0, 350.0, (n, 2))
    s_major = rng.uniform(20.0, 45.0, n)
    ratio = np.where(kind == 10, 1.0, rng.uniform(1.5, 3.0, n))
    s_minor = s_major / ratio
    theta = rng.uniform(0.0, np.pi, n)
    peak = rng.uniform(60.0, 100.0, n)
    i = np.arange(k)[None, :]
    rad = rng.uniform(0.5, 2.0, (n, k))
    ang = rng.uniform(0.0, 2.0 * np.pi, (n, k))
    tke = rng.uniform(0.0, 6.0, (n, k))
    # few usable records: all but the first m of the records i = 1 (mod 3) stand 4 .. 4.5 sigma away, where b < 0.04
    m = np.select([kind == 7, kind == 8, kind == 9], [0, 5, 8], -1)[:, None]
    nth = np.cumsum(i % 3 == 1, axis=1) * (i % 3 == 1)
    far = (m >= 0) & ~((nth >= 1) & (nth <= m))
    rad = np.where(far, rng.uniform(4.0, 4.5, (n, k)), rad)
    # clipped cells: every third record within 0.1 sigma with tke 8 under a peak of 100, so that plume + tke > 100
    close = (kind == 11)[:, None] & (i % 3 == 0)
    peak = np.where(kind == 11, 100.0, peak)
    rad = np.where(close, rng.uniform(0.0, 0.1, (n, k)), rad)
    tke = np.where(close, 8.0, tke)
    u, v = rad * np.cos(ang) * s_major[:, None], rad * np.sin(ang) * s_minor[:, None]
    cs, sn = np.cos(theta)[:, None], np.sin(theta)[:, None]
    off = np.stack([u * cs - v * sn, u * sn + v * cs], 2)
    line = kind == 4                                                        # one row of cells: q is constant
    off[line, :, 0] = s_minor[line, None] * rng.uniform(-1.5, 1.5, (int(line.sum()), k))
    off[line, :, 1] = 0.5 * s_minor[line, None]
    pos = (src[:, None, :] + off).astype(np.float32)
    # the end of the episode
    p = np.minimum(k - 1, 40 + (e // K) * 5 % max(k - 40, 1))
    flags = np.zeros((n, k), np.uint8)
    code = np.select([kind == 0, kind == 1, kind == 3], [1 | 2, 8, 1], 0)
    has_end = np.isin(kind, (0, 1, 3))
    flags[e[has_end], p[has_end]] = code[has_end]
    tail_end = np.isin(kind, (4, 5, 6))
    flags[tail_end, k - 1] = 1
    behind = i > p[:, None]
    skipped = behind & (kind == 0)[:, None]
    flags[skipped] = 4
    other = behind & (kind == 1)[:, None]                                   # stepped records behind a bit3 end: never to be used
    pos = np.where(other[:, :, None], pos + np.float32(60.0), pos).astype(np.float32)
    base = ellipse_field(src, s_major, s_minor, theta, peak)

    def field_of(c):
        f = base(c)
        dx, dy = (c[:, :, 0] - src[:, None, 0]) / s_major[:, None], (c[:, :, 1] - src[:, None, 1]) / s_major[:, None]
        f = np.where((kind == 5)[:, None], 10.0 * np.exp(0.5 * dx * dx - 0.5 * dy * dy), f)        # falls along y, rises along x
        return np.where((kind == 6)[:, None], 2.0 * np.exp(0.5 * (dx * dx + dy * dy)), f)          # rises outwards
    obs = _records(pos, field_of, tke, D, rng)
    obs[skipped] = NAN
    pos[skipped] = NAN
    ended = np.where(kind == 3, np.where(e % 24 == 3, 1, 3), 0).astype(np.uint8)
    state = np.zeros((n, 33), np.float64)
    gone = kind == 3
    state[gone] = 0.5 + np.arange(33 * int(gone.sum()), dtype=np.float64).reshape(-1, 33)
    return {"flags": flags, "obs": obs, "pos": pos, "ended": ended, "state": state, "src": src, "kind": kind,
            "truth": np.stack([s_major, s_minor, theta, peak], 1)}


def estimates6(n, seed=0):
    """(est f64 [n, 10], status u8 [n], src f64 [n, 2], truth f64 [n, 4]) for uav_source_summary6: every status, estimates some
    within a few cells of the source and some not, envs without a largest sample (count 0: all ten NaN), truth rows with a NaN."""
    rng = np.random.default_rng(177 + seed + n)
    src = rng.uniform(100.0, 400.0, (n, 2))
    status = (np.arange(n) % 5 % 4).astype(np.uint8)
    truth = np.stack([rng.uniform(20.0, 45.0, n), rng.uniform(8.0, 20.0, n), rng.uniform(0.0, np.pi, n), rng.uniform(60.0, 100.0, n)], 1)
    est = np.empty((n, 10), np.float64)
    est[:, 0:2] = src + rng.normal(0.0, 4.0, (n, 2))
    est[:, 2:4] = truth[:, 0:2] * rng.uniform(0.9, 1.1, (n, 2))
    est[:, 4] = np.mod(truth[:, 2] + rng.uniform(-2.0, 2.0, n), np.pi)
    est[:, 5] = truth[:, 3] * rng.uniform(0.9, 1.1, n)
    est[:, 6] = 2.0 * np.pi * est[:, 2] * est[:, 3] * est[:, 5]
    est[:, 7:9] = np.floor(src + rng.normal(0.0, 30.0, (n, 2)))
    est[:, 9] = rng.uniform(1.0, 99.0, n)
    est[status != 0, 0:7] = NAN
    empty = (status == 1) & (np.arange(n) % 3 == 0)
    est[empty] = NAN
    truth[np.arange(n) % 7 == 0, np.arange(n)[np.arange(n) % 7 == 0] % 4] = NAN      # one NaN somewhere in the row
    truth[np.arange(n) % 11 == 5] = NAN
    if n > 7:
        est[5, 0:2] = src[5] + np.array([3.0, 4.0])                        # 3-4-5: the error equals a loc_tol of 5 exactly
    return est, status, src, truth
