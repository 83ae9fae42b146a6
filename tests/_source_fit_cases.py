"""Synthetic greedy records for the source estimator, shared by tests/test_source_fit_host.py and tests/test_gpu_source_fit.py:
E3's formula (csrc/env_core.h field_at: 100 exp(-d^2 / 2 sigma^2) + tke, clipped to 0 .. 100) restated in numpy, sampled by walkers
around random sources.  obs is f32 as the kernels write it; the obs / pos of every bit2 (not stepped) record are NaN."""
import numpy as np

NAN = float("nan")
KINDS = ("ends by bit0", "ends by bit3, stepped records of another plume behind it", "ends by bit0 and bit3", "ends nowhere",
         "comes in ended", "clipped cells", "collinear track", "bowl", "0 usable records", "3 usable records", "4 usable records",
         "5 usable records")
K = len(KINDS)
# uav_source_solve's status where the chunk is long enough for the kind to show (k >= MIN_K), min_samples = 5; None: not solved
FITTED, FEW, DEGENERATE, NOT_A_PEAK = 0, 1, 2, 3
EXPECTED = (FITTED, FITTED, FITTED, FITTED, None, FITTED, DEGENERATE, NOT_A_PEAK, FEW, FEW, FEW, FITTED)
MIN_K = 24


def cells(pos):
    return np.fmin(np.fmax(pos.astype(np.float32), np.float32(0.0)), np.float32(499.0)).astype(np.int32)


def episodes(n, k, D, seed=0):
    """dict(flags u8 [n, k], obs f32 [n, k, D], pos f32 [n, k, 2], ended u8 [n], state f64 [n, 20] (the start state: zeros, and
    sentinels in the envs that come in ended), src f64 [n, 2], sigma f64 [n], kind i64 [n]).  Env e is of kind KINDS[e % 12]."""
    rng = np.random.default_rng(1000003 * seed + 1009 * n + 17 * k + D)
    e = np.arange(n)
    kind = e % K
    src = rng.uniform(150.0, 350.0, (n, 2))
    sigma = np.where(rng.integers(0, 2, n) == 0, 500.0 / 16.0, 15.0)
    i = np.arange(k)[None, :]
    # walkers: radius 0.6 .. 2.4 sigma around the source, any direction
    rad = sigma[:, None] * rng.uniform(0.6, 2.4, (n, k))
    ang = rng.uniform(0.0, 2.0 * np.pi, (n, k))
    tke = rng.uniform(0.0, 6.0, (n, k))
    # few usable records: all but the first m of the records i = 1 (mod 3) stand 4 .. 4.5 sigma away, where b < 0.04
    m = np.select([kind == 8, kind == 9, kind == 10, kind == 11], [0, 3, 4, 5], -1)[:, None]
    nth = np.cumsum(i % 3 == 1, axis=1) * (i % 3 == 1)                   # 1, 2, ... at the records 1, 4, 7, ...
    far = (m >= 0) & ~((nth >= 1) & (nth <= m))
    rad = np.where(far, sigma[:, None] * rng.uniform(4.0, 4.5, (n, k)), rad)
    # clipped cells: every third record within 0.2 sigma with tke 8, so that plume + tke > 100
    close = (kind == 5)[:, None] & (i % 3 == 0)
    rad = np.where(close, sigma[:, None] * rng.uniform(0.0, 0.2, (n, k)), rad)
    tke = np.where(close, 8.0, tke)
    off = np.stack([rad * np.cos(ang), rad * np.sin(ang)], 2)
    line = kind == 6                                                        # one row of cells: q is constant
    off[line, :, 0] = sigma[line, None] * rng.uniform(-2.0, 2.0, (int(line.sum()), k))
    off[line, :, 1] = 0.7 * sigma[line, None]
    pos = (src[:, None, :] + off).astype(np.float32)
    # the end of the episode
    p = np.minimum(k - 1, 8 + (e // K) * 5 % max(k - 8, 1))
    flags = np.zeros((n, k), np.uint8)
    code = np.select([kind == 0, kind == 1, kind == 2, kind == 4], [1 | 2, 8, 9, 1], 0)
    has_end = np.isin(kind, (0, 1, 2, 4))
    flags[e[has_end], p[has_end]] = code[has_end]
    tail_end = np.isin(kind, (5, 6, 7))
    flags[tail_end, k - 1] = 1
    behind = i > p[:, None]
    skipped = behind & np.isin(kind, (0, 2))[:, None]
    flags[skipped] = 4
    other = behind & (kind == 1)[:, None]                                   # stepped records behind a bit3 end: never to be used
    pos = np.where(other[:, :, None], pos + np.float32(60.0), pos).astype(np.float32)
    # the field at the cell of the position
    c = cells(pos).astype(np.float64)
    d2 = (c[:, :, 0] - src[:, None, 0]) ** 2 + (c[:, :, 1] - src[:, None, 1]) ** 2
    plume = 100.0 * np.exp(-d2 / (2.0 * sigma[:, None] ** 2))
    plume = np.where((kind == 7)[:, None], 2.0 * np.exp(d2 / (2.0 * sigma[:, None] ** 2)), plume)      # rising outwards
    conc = np.clip(plume + tke, 0.0, 100.0)
    obs = rng.uniform(0.0, 1.0, (n, k, D)).astype(np.float32)
    obs[:, :, 0:2] = pos / np.float32(500.0)
    obs[:, :, 2] = (conc / 100.0).astype(np.float32)
    obs[:, :, 3] = (tke / 9.0).astype(np.float32)
    obs[skipped] = NAN
    pos[skipped] = NAN
    ended = np.where(kind == 4, np.where(e % 24 == 4, 1, 3), 0).astype(np.uint8)
    state = np.zeros((n, 20), np.float64)
    gone = kind == 4
    state[gone] = 0.5 + np.arange(20 * int(gone.sum()), dtype=np.float64).reshape(-1, 20)
    return {"flags": flags, "obs": obs, "pos": pos, "ended": ended, "state": state, "src": src, "sigma": sigma, "kind": kind}


def estimates(n, seed=0):
    """(est f64 [n, 8], status u8 [n], src f64 [n, 2]) for uav_source_summary: every status, estimates some within a few cells of
    the source and some not, envs without a largest sample (count 0: all eight NaN)."""
    rng = np.random.default_rng(77 + seed + n)
    src = rng.uniform(100.0, 400.0, (n, 2))
    status = (np.arange(n) % 5 % 4).astype(np.uint8)
    est = np.empty((n, 8), np.float64)
    est[:, 0:2] = src + rng.normal(0.0, 4.0, (n, 2))
    est[:, 2] = rng.uniform(10.0, 40.0, n)
    est[:, 3] = rng.uniform(50.0, 150.0, n)
    est[:, 4] = 2.0 * np.pi * est[:, 2] ** 2 * est[:, 3]
    est[:, 5:7] = np.floor(src + rng.normal(0.0, 30.0, (n, 2)))
    est[:, 7] = rng.uniform(1.0, 99.0, n)
    est[status != 0, 0:5] = NAN
    empty = (status == 1) & (np.arange(n) % 3 == 0)
    est[empty] = NAN
    if n > 7:
        est[5, 0:2] = src[5] + np.array([3.0, 4.0])                        # 3-4-5: the error equals a loc_tol of 5 exactly
    return est, status, src
