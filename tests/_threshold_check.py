"""numpy restatement of uav_threshold_windows / uav_threshold_rule (csrc/threshold.hip), shared by tests/test_threshold_host.py
and tests/test_gpu_threshold_scan.py.  Everything is float64 on float32 inputs, one operation at a time, as the kernels do it."""
import numpy as np

CONC_SCALE, FACTOR = 100.0, 0.95
REFERENCE = dict(window=10, every=10, min_steps=20)


def np_order_mean(a):
    """np.mean of a short f64 run, restated: add.reduce sums fewer than 8 values one by one and up to 128 in eight interleaved
    accumulators combined pairwise, the remainder added behind (numpy's pairwise_sum, below its blocking size)."""
    a = np.asarray(a, np.float64)
    w = len(a)
    assert 1 <= w <= 128
    if w < 8:
        res = np.float64(0.0)
        for v in a:
            res = res + v
    else:
        r = [a[j] for j in range(8)]
        i = 8
        while i < w - w % 8:
            for j in range(8):
                r[j] = r[j] + a[i + j]
            i += 8
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        while i < w:
            res = res + a[i]
            i += 1
    return res / np.float64(w)


def slots(steps, every):
    return (steps + every - 1) // every


def _seq(series, hist, cnt, e, window):
    fill = min(int(cnt[e]), window - 1)
    return fill, np.concatenate([hist[e, :fill], series[e]]).astype(np.float32)


def is_update(t, window, every, min_steps):
    return t % every == 0 and t >= max(window, min_steps)


def windows_ref(series, hist, cnt, active=None, window=10, every=10, min_steps=20, lo=0.0, scale=1.0, conc_scale=CONC_SCALE):
    """uav_threshold_windows: x f32 [n, S, window]"""
    n, steps = series.shape
    active = np.ones(n, bool) if active is None else np.asarray(active, bool)
    x = np.zeros((n, slots(steps, every), window), np.float32)
    for e in range(n):
        if not active[e]:
            continue
        fill, seq = _seq(series, hist, cnt, e, window)
        for i in range(steps):
            t = int(cnt[e]) + i + 1
            if is_update(t, window, every, min_steps):
                s = t // every - int(cnt[e]) // every - 1
                v = seq[fill + i + 1 - window:fill + i + 1].astype(np.float64)
                x[e, s] = ((v * np.float64(conc_scale) - np.float64(lo)) / np.float64(scale)).astype(np.float32)
    return x


def rule_ref(series, hist, cnt, pred, thr, active=None, window=10, every=10, min_steps=20, conc_scale=CONC_SCALE, factor=FACTOR,
             met=None):
    """uav_threshold_rule: (first_hit i32 [n], stop u8 [n, steps], thr_out f64 [n, steps], thr, hist, cnt on exit).
    met (a list) collects (env, step, |cur - thr|, |mean - thr| or inf) of every step at which the rule compared."""
    n, steps = series.shape
    active = np.ones(n, bool) if active is None else np.asarray(active, bool)
    first = np.full(n, -1, np.int32)
    stop = np.zeros((n, steps), np.uint8)
    thr_out = np.repeat(np.asarray(thr, np.float64)[:, None], steps, 1)
    thr_x, hist_x, cnt_x = np.array(thr, np.float64), hist.copy(), np.array(cnt, np.int32)
    for e in range(n):
        if not active[e]:
            continue
        fill, seq = _seq(series, hist, cnt, e, window)
        th = np.float64(thr[e])
        for i in range(steps):
            t = int(cnt[e]) + i + 1
            if is_update(t, window, every, min_steps):
                th = np.float64(pred[e, t // every - int(cnt[e]) // every - 1]) * np.float64(factor)
            cur = np.float64(series[e, i]) * np.float64(conc_scale)
            hit = False
            if t >= min_steps and not np.isnan(th):
                mean = np.float64(np.nan)
                if t >= window:
                    mean = np_order_mean(seq[fill + i + 1 - window:fill + i + 1].astype(np.float64) * np.float64(conc_scale))
                hit = bool(cur >= th) or bool(mean >= th)          # a NaN compares false
                if met is not None:
                    met.append((e, i, abs(cur - th), abs(mean - th) if t >= window else np.inf))
            stop[e, i] = hit
            thr_out[e, i] = th
            if hit and first[e] < 0:
                first[e] = i
        thr_x[e] = th
        tail = seq[len(seq) - min(len(seq), window - 1):] if window > 1 else seq[:0]
        hist_x[e, :len(tail)] = tail
        cnt_x[e] = int(cnt[e]) + steps
    return first, stop, thr_out, thr_x, hist_x, cnt_x


def live_margin(met, first, upto=None):
    """The smallest |cur - thr| / |mean - thr| the rule met while each env's episode was live: steps up to and including its first
    hit (`upto[e]` caps that, e.g. at the env's first done record).  NaN distances (NaN inputs) are skipped."""
    m = np.inf
    for e, i, dc, dm in met:
        end = first[e] if first[e] >= 0 else np.inf
        if upto is not None:
            end = min(end, upto[e])
        if i <= end:
            for d in (dc, dm):
                if not np.isnan(d):
                    m = min(m, d)
    return m
