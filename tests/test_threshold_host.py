"""uav_threshold_windows / uav_threshold_rule (csrc/threshold.hip) as far as they go without a GPU: the numpy restatement the GPU
tests compare against (tests/_threshold_check.py) is itself pinned here -- its mean to np.mean bit for bit, the whole rule to the
reference's recorded ThresholdController traces (tests/golden/eval_v20.npz) -- and the refusals of the built library, which are
answered before any device is touched."""
import ctypes as C
import os

import numpy as np
import pytest

from _threshold_check import FACTOR, REFERENCE, live_margin, np_order_mean, rule_ref, slots, windows_ref
from oracle import eval_oracle as eo

GOLD = os.path.join(os.path.dirname(__file__), "golden", "eval_v20.npz")


@pytest.mark.parametrize("w", [1, 3, 7, 8, 9, 10, 15, 16, 20, 31, 32])
def test_restated_mean_is_np_mean_bit_for_bit(w):
    """The reference calls np.mean on a Python list of floats; a plain sequential sum differs from it on about a quarter of the
    windows at w = 10 (asserted, so that this test could tell the two apart)."""
    rng = np.random.RandomState(w)
    sets = np.concatenate([rng.uniform(0.0, 100.0, (4000, w)), np.exp(rng.uniform(np.log(1e-6), np.log(1e3), (1000, w)))])
    seq_differs = 0
    for a in sets:
        want = np.mean(list(a))
        got = np_order_mean(a)
        assert got == want and np.float64(got).tobytes() == np.float64(want).tobytes(), (w, a)
        s = np.float64(0.0)
        for v in a:
            s = s + v
        seq_differs += (s / np.float64(w)) != want
    if w == 10:
        assert seq_differs > 0.1 * len(sets), seq_differs


def _golden():
    g = np.load(GOLD, allow_pickle=False)
    sd = {k[3:]: g[k] for k in g.files if k.startswith("sd/")}
    lo, hi = float(g["scaler_params"].min()), float(g["scaler_params"].max())
    return g, eo.ThresholdPredictorOracle(sd), lo, (hi - lo) if hi != lo else 1.0


def golden_scan(cuts):
    """The restated kernels over the golden's 8 recorded trajectories, f32(traj / 100) as the series, in calls of `cuts` steps"""
    g, onet, lo, scale = _golden()
    series = (g["traj"] / 100.0).astype(np.float32)
    E, L = series.shape
    assert sum(cuts) == L
    hist, cnt, thr = np.zeros((E, 9), np.float32), np.zeros(E, np.int32), np.full(E, np.nan)
    first, thr_steps, met, t0 = np.full(E, -1), [], [], 0
    for k in cuts:
        part = series[:, t0:t0 + k]
        x = windows_ref(part, hist, cnt, lo=lo, scale=scale, **REFERENCE)
        pred = onet(x.reshape(-1, 10, 1)).numpy().reshape(E, slots(k, 10))
        part_met = []
        f, _, thr_out, thr, hist, cnt = rule_ref(part, hist, cnt, pred, thr, met=part_met, **REFERENCE)
        met += [(e, i + t0, a, b) for e, i, a, b in part_met]
        first = np.where((first < 0) & (f >= 0), f + t0, first)
        thr_steps.append(thr_out)
        t0 += k
    return g, first, np.concatenate(thr_steps, 1), met


@pytest.mark.parametrize("cuts", [(90,), (50, 40), (17,) * 5 + (5,)])
def test_restatement_reproduces_the_reference_golden(cuts):
    g, first, thr_out, met = golden_scan(cuts)
    stop_at = np.where(first >= 0, first + 1, -1)
    assert np.array_equal(stop_at, g["stop_at"]), (stop_at, g["stop_at"])
    assert np.array_equal(stop_at, [-1, -1, -1, 48, 48, -1, 51, 52])
    want = g["thresholds"]
    checked, worst = 0, 0.0
    for e in range(want.shape[0]):
        for j in range(want.shape[1]):
            step = 10 * (j + 1)
            if np.isnan(want[e, j]) or (first[e] >= 0 and step > first[e] + 1):
                continue
            err = abs(thr_out[e, step - 1] - want[e, j])
            assert err < 2e-3 * max(1.0, abs(want[e, j])), (e, step, err)             # tests/test_gpu_eval.py's bound
            worst = max(worst, err)
            checked += 1
    assert checked > 40 and np.isnan(thr_out[:, :19]).all() and not np.isnan(thr_out[:, 19:]).any()
    margin = live_margin(met, first)
    print(f"cuts {cuts}: {checked} thresholds, worst error {worst:.3g}; smallest live |cur - thr| or |mean - thr| {margin:.3g}")
    # the decisions above are no accident of rounding: the closest call of a live episode is far from the predictor's f32 error
    assert margin > 1e-2, margin


def test_windows_of_the_golden_are_the_hosts_scaled_slices():
    """x is ((window - lo) / scale).to(float32) of the last 10 concentrations f64(f32(traj / 100)) * 100 at steps 20, 30, ..; zero
    rows for the slot of step 10 (before min_steps)."""
    g, _, lo, scale = _golden()
    series = (g["traj"] / 100.0).astype(np.float32)
    E, L = series.shape
    x = windows_ref(series, np.zeros((E, 9), np.float32), np.zeros(E, np.int32), lo=lo, scale=scale, **REFERENCE)
    assert x.shape == (E, 9, 10) and not x[:, 0].any()
    conc = series.astype(np.float64) * 100.0
    for s in range(1, 9):
        t = 10 * (s + 1)
        assert np.array_equal(x[:, s], ((conc[:, t - 10:t] - lo) / scale).astype(np.float32))


# ---------------------------------------------------------------------------------------------- refusals, no device
@pytest.fixture(scope="module")
def lib():
    from uavppo import _lib
    return _lib.lib()


def _call(lib, which, window=10, every=10, steps=5, n=3, null=(), handle=None):
    """Host buffers standing in for device ones: every case here is refused before a pointer is followed."""
    bufs = {k: (C.c_float * 4096)() for k in ("series", "hist", "x", "pred")}
    bufs.update({k: (C.c_int32 * 16)() for k in ("step_cnt", "first_hit")})
    bufs["thr"] = (C.c_double * 16)()
    a = {k: (None if k in null else C.cast(v, C.c_void_p)) for k, v in bufs.items()}
    if which == "windows":
        return lib.uav_threshold_windows(handle, a["series"], steps, 1, n, steps, None, a["hist"], a["step_cnt"], window, every, 20,
                                         0.0, 1.0, 100.0, a["x"], None)
    return lib.uav_threshold_rule(handle, a["series"], steps, 1, n, steps, None, a["hist"], a["step_cnt"], window, every, 20, 100.0,
                                  FACTOR, a["pred"], a["thr"], a["first_hit"], None, None, None)


COMMON = [({"window": 0}, b"window=0"), ({"window": 33}, b"window=33"), ({"every": 0}, b"every=0"), ({"n": 0}, b"n=0"),
          ({"steps": 0}, b"steps=0"), ({"null": ("series",)}, b"NULL series"), ({"null": ("hist",)}, b"NULL hist"),
          ({"null": ("step_cnt",)}, b"step_cnt"), ({}, b"NULL handle")]


@pytest.mark.parametrize("kw,word", COMMON + [({"null": ("x",)}, b"NULL x")])
def test_windows_refuses_with_a_reason_and_without_a_device(lib, kw, word):
    rc = _call(lib, "windows", **kw)
    err = lib.uav_last_error()
    assert rc != 0 and b"uav_threshold_windows" in err and word in err, (rc, err)


@pytest.mark.parametrize("kw,word", COMMON + [({"null": ("pred",)}, b"NULL pred"), ({"null": ("thr",)}, b"NULL thr"),
                                              ({"null": ("first_hit",)}, b"NULL first_hit")])
def test_rule_refuses_with_a_reason_and_without_a_device(lib, kw, word):
    rc = _call(lib, "rule", **kw)
    err = lib.uav_last_error()
    assert rc != 0 and b"uav_threshold_rule" in err and word in err, (rc, err)


def test_device_threshold_skips_the_predictor_where_no_update_step_can_fall():
    """_DeviceThreshold.has_update(t0, k): is there a t in (t0, t0 + k] with t % 10 == 0 and t >= max(window, min_steps)"""
    import evaluate_with_lstm as ev

    class Ctl:
        model, lo, scale, window_size, min_activate_steps = None, 0.0, 1.0, 10, 20

    d = ev._DeviceThreshold(Ctl, 2, "cpu")
    for t0 in range(0, 45):
        for k in (1, 3, 10, 17, 50):
            want = any(t % 10 == 0 and t >= 20 for t in range(t0 + 1, t0 + k + 1))
            assert d.has_update(t0, k) == want, (t0, k)
    Ctl.window_size = 33
    with pytest.raises(RuntimeError, match="window_size = 33"):
        ev._DeviceThreshold(Ctl, 2, "cpu")
