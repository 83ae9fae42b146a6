"""uav_peak_stop_param_count / uav_peak_stop_scan (csrc/peak_stop.hip) as far as they go without a GPU: the parameter count, the
refusals (answered before any device is touched), PeakAndStopPredictor.flat_params() and the identity the kernel rests on -- the
host loop's f32((f64(obs2) * 100) / 100) is obs2 bit for bit, so the kernel may read obs[2] of the records as it is."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "uav-wrf-les-ppo-lstm_amd")


@pytest.fixture(scope="module")
def lib():
    from uavppo import _lib
    return _lib.lib()


def test_param_count(lib):
    H = 32
    assert lib.uav_peak_stop_param_count(H) == 4546 == 4 * H + 4 * H * H + 4 * H + 4 * H + H + 1 + H + 1
    assert lib.uav_peak_stop_param_count(48) == 0
    err = lib.uav_last_error()
    assert err and b"uav_peak_stop_param_count" in err and b"hidden=48" in err, err


def _scan(lib, hidden=32, window=20, steps=5, n=3, null=()):
    """The call with host buffers standing in for device ones: every case here is refused before a pointer is followed."""
    bufs = {k: (C.c_float * 4600)() for k in ("params", "series", "hist", "peak", "prob")}
    bufs.update({k: (C.c_int32 * 16)() for k in ("hist_cnt", "first_hit")})
    a = {k: (None if k in null else C.cast(v, C.c_void_p)) for k, v in bufs.items()}
    return lib.uav_peak_stop_scan(None, a["params"], hidden, window, a["series"], steps, 1, n, steps, None, a["hist"], a["hist_cnt"],
                                  0.8, a["peak"], a["prob"], a["first_hit"], None)


@pytest.mark.parametrize("kw,word", [({"hidden": 48}, b"hidden=48"), ({"window": 0}, b"window=0"), ({"window": 33}, b"window=33"),
                                     ({"steps": 0}, b"steps=0"), ({"n": 0}, b"n=0"), ({"null": ("hist",)}, b"NULL hist"),
                                     ({"null": ("hist_cnt",)}, b"NULL hist"), ({"null": ("params",)}, b"NULL params"),
                                     ({"null": ("series",)}, b"NULL params / series"), ({"null": ("first_hit",)}, b"NULL first_hit"),
                                     ({}, b"NULL handle")])
def test_scan_refuses_with_a_reason_and_without_a_device(lib, kw, word):
    rc = _scan(lib, **kw)
    err = lib.uav_last_error()
    assert rc != 0 and b"uav_peak_stop_scan" in err and word in err, (rc, err)


def test_flat_params_is_the_state_dict_in_order():
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    import evaluate_with_lstm as ev
    pred = ev.PeakAndStopPredictor(device="cpu", seed=3)
    flat = pred.flat_params()
    sd = pred.state_dict()
    keys = ["lstm.weight_ih_l0", "lstm.weight_hh_l0", "lstm.bias_ih_l0", "lstm.bias_hh_l0", "fc_peak.weight", "fc_peak.bias",
            "fc_stop.0.weight", "fc_stop.0.bias"]
    assert list(sd) == keys
    assert [tuple(sd[k].shape) for k in keys] == [(128, 1), (128, 32), (128,), (128,), (1, 32), (1,), (1, 32), (1,)]
    assert flat.dtype == torch.float32 and flat.shape == (4546,) and flat.is_contiguous()
    assert torch.equal(flat, torch.cat([sd[k].reshape(-1) for k in keys]))
    assert ev.peak_stop_refusal(pred, 20) is None
    assert "hidden 48" in ev.peak_stop_refusal(ev.PeakAndStopPredictor(hidden_dim=48, device="cpu"), 20)
    assert "2 layer" in ev.peak_stop_refusal(ev.PeakAndStopPredictor(num_layers=2, device="cpu"), 20)
    assert "input_dim 3" in ev.peak_stop_refusal(ev.PeakAndStopPredictor(input_dim=3, device="cpu"), 20)
    assert "window_size_v21 = 33" in ev.peak_stop_refusal(pred, 33)


def test_times_100_over_100_round_trip_is_the_identity_on_f32():
    """evaluate()'s host loop keeps obs[2] as f64(obs2) * 100 and feeds f32(that / 100).  x * 100 rounds to f64 with relative error
    <= 2^-53, the quotient adds as much: the result is within 2^-52 relative of the f32 value x, far inside its rounding cell."""
    rng = np.random.RandomState(0)
    sets = [rng.uniform(0.0, 1.5, 4_000_000).astype(np.float32),
            np.exp(rng.uniform(np.log(1e-30), np.log(10.0), 2_000_000)).astype(np.float32),
            np.array([0.0, 1.0, 1.5, np.float32(1e-38), np.float32(1e-45), np.finfo(np.float32).max / 200], np.float32)]
    for x in sets:
        back = ((x.astype(np.float64) * 100.0) / 100.0).astype(np.float32)
        assert np.array_equal(back, x)
    t = torch.from_numpy(sets[0])
    assert torch.equal(((t.to(torch.float64) * 100.0) / 100.0).to(torch.float32), t)          # the same through torch's casts
