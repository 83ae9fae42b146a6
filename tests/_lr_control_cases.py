"""The hand-written table of adapt_rule cases that tests/test_lr_control_host.py checks in numpy and tests/test_gpu_lr_control.py
runs through uav_lr_adapt, and the random rows of the latter."""
import numpy as np

NAN, INF = float("nan"), float("inf")
D, F, LO, HI = 0.01, 1.5, 1e-6, 1e-2            # desired_kl, factor, lr_min, lr_max of the table


def sums(kl_sum, n, fill=0.0):
    """Eight diagnostic sums with S[1] = kl_sum, S[7] = n (ops.PPO_DIAG_NAMES)."""
    s = np.full(8, fill, dtype=np.float64)
    s[1], s[7] = kl_sum, n
    return s


# name, lr before, sums8, lr after, the slot counted.  n = 1024 is a power of two: kl = S[1] / n is exact, so the edges are exact.
TABLE = [
    ("above 2 x desired", 3e-5, sums(0.021 * 1024, 1024), 3e-5 / 1.5, "lowered"),
    ("below desired / 2", 3e-5, sums(0.004 * 1024, 1024), 3e-5 * 1.5, "raised"),
    ("exactly 2 x desired holds", 3e-5, sums(2 * D * 1024, 1024), 3e-5, "held"),
    ("exactly desired / 2 holds", 3e-5, sums(D / 2 * 1024, 1024), 3e-5, "held"),
    ("inside the band", 3e-5, sums(0.01 * 1024, 1024), 3e-5, "held"),
    ("zero kl raises", 3e-5, sums(0.0, 1024), 3e-5 * 1.5, "raised"),
    ("NaN sum", 3e-5, sums(NAN, 1024), 3e-5, "skipped"),
    ("+inf sum", 3e-5, sums(INF, 1024), 3e-5 / 1.5, "lowered"),
    ("n = 0", 3e-5, sums(0.5, 0.0), 3e-5, "skipped"),
    ("n = 0 and no sum (0 / 0)", 3e-5, sums(0.0, 0.0), 3e-5, "skipped"),
    ("n is a NaN", 3e-5, sums(0.5, NAN), 3e-5, "skipped"),
    ("clamp at lr_min", 1.2e-6, sums(1.0 * 1024, 1024), LO, "lowered"),
    ("clamp at lr_max", 9e-3, sums(0.0, 1024), HI, "raised"),
    ("other sums are not read", 3e-5, sums(0.021 * 1024, 1024, fill=NAN), 3e-5 / 1.5, "lowered"),
]


def random_rows(count, seed=7):
    """(state f64 [6], sums8 f64 [8], desired_kl, factor, lr_min, lr_max) x count: rates and KLs over many decades, one row in
    eight with a NaN / inf / empty batch."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        lo = 10.0 ** rng.uniform(-8, -4)
        hi = lo * 10.0 ** rng.uniform(0, 4)
        lr = min(max(lo * 10.0 ** rng.uniform(0, 4), lo), hi)
        state = np.array([lr, rng.uniform(0, 1), *rng.integers(0, 50, 4)], dtype=np.float64)
        desired = 10.0 ** rng.uniform(-4, -1)
        n = float(rng.integers(1, 1 << 20))
        s = rng.standard_normal(8)
        s[1], s[7] = desired * n * 10.0 ** rng.uniform(-1, 1), n
        if i % 8 == 7:
            k = (i // 8) % 4
            s[1], s[7] = ((NAN, n), (INF, n), (s[1], 0.0), (-INF, n))[k]
        out.append((state, s.astype(np.float64), desired, rng.uniform(1.01, 3.0), lo, hi))
    return out
