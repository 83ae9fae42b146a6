"""N3: offline training of the stop predictor on the GPU vs the training oracle (pinned to the reference's
loop body by tests/test_oracle_train_lstm.py).  -m gpu."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import lstm_train_oracle as lt

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(__file__), "golden", "train_lstm_v20.npz")


@pytest.fixture(scope="module")
def tl():
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "uav-wrf-les-ppo-lstm_amd")
    if root not in sys.path:
        sys.path.insert(0, root)
    import train_lstm as m
    return m


def _seqs(g):
    out, o = [], 0
    for L in g["seq_lens"]:
        out.append(list(g["seq_flat"][o:o + L]))
        o += L
    return out


def test_sequence_dataset_matches_reference_golden(tl):
    g = np.load(GOLD, allow_pickle=False)
    ds = tl.SequenceDataset(_seqs(g), g["source_concs"], int(g["training_size"]))
    assert np.allclose(ds.windows, g["X"], atol=1e-6) and np.allclose(ds.labels, g["Y"], atol=1e-6)
    assert np.isclose(ds.data_min_[0], g["data_min"][0]) and np.isclose(ds.data_max_[0], g["data_max"][0])
    x0, y0 = ds[3]
    assert x0.shape == (int(g["training_size"]),) and y0.shape == (1,)


def test_three_eval_mode_steps_match_the_reference_golden(tl):
    """The reference's model / SmoothL1Loss / clip / AdamW for three steps (eval mode), replayed on the GPU kernels."""
    from evaluate_with_lstm import ConcentrationThresholdPredictor
    g = np.load(GOLD, allow_pickle=False)
    model = ConcentrationThresholdPredictor(hidden_size=32, device=DEV)
    model.load_state_dict({k[5:]: g[k] for k in g.files if k.startswith("init/")})
    tr = tl.PredictorTrainer(model, lr=3e-4)
    x = torch.from_numpy(g["X"][:24]).to(DEV)[:, :, None].contiguous()
    y = torch.from_numpy(g["Y"][:24]).to(DEV)
    for k in range(3):
        loss = tr.train_step(x, y, masks=None)
        assert np.isclose(float(loss.item()), g["losses"][k], rtol=2e-5), (k, float(loss.item()), g["losses"][k])
        assert np.isclose(float(tr.gnorm.item()), g["gnorms"][k], rtol=2e-4)
    for k, v in model.state_dict().items():
        want = g["post/" + k]
        assert np.allclose(v.cpu().numpy(), want, rtol=2e-3, atol=3e-6), k      # Adam turns 1e-6 gradient noise into ~1e-6 steps


def test_three_steps_on_ragged_sequences_match_the_reference_golden(tl):
    """model.py:229-240's forward(x, lengths) in the training loop: three optimiser steps on zero-padded ragged sequences
    (lengths 1..10) against the reference's own packed-sequence run; and, with dropout masks, against the oracle."""
    from evaluate_with_lstm import ConcentrationThresholdPredictor
    g = np.load(GOLD, allow_pickle=False)
    model = ConcentrationThresholdPredictor(hidden_size=32, device=DEV)
    model.load_state_dict({k[5:]: g[k] for k in g.files if k.startswith("init/")})
    tr = tl.PredictorTrainer(model, lr=3e-4)
    x = torch.from_numpy(g["ragged_x"]).to(DEV)[:, :, None].contiguous()
    y = torch.from_numpy(g["Y"][:24]).to(DEV)
    lens = g["ragged_lengths"]
    for k in range(3):
        loss = tr.train_step(x, y, masks=None, lengths=lens)
        assert np.isclose(float(loss.item()), g["ragged_losses"][k], rtol=2e-5), (k, float(loss.item()), g["ragged_losses"][k])
        assert np.isclose(float(tr.gnorm.item()), g["ragged_gnorms"][k], rtol=2e-4)
    for k, v in model.state_dict().items():
        assert np.allclose(v.cpu().numpy(), g["ragged_post/" + k], rtol=2e-3, atol=3e-6), k
    with pytest.raises(ValueError):
        tr.train_step(x, y, lengths=[0] * 24)
    # dropout masks + ragged lengths against the oracle
    params = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    opt = lt.AdamWState(params, lr=3e-4)
    opt.t, opt.m, opt.v = 3, {}, {}
    o = 0
    names = [(f"lstm.{k}", v) for k, v in model.lstm.p.items()] + list(model.fc.items())
    for name, v in names:                                      # the trainer's Adam state, cut into the oracle's tensors
        n = v.numel()
        opt.m[name] = tr.exp_avg[o:o + n].view(v.shape).cpu().clone()
        opt.v[name] = tr.exp_avg_sq[o:o + n].view(v.shape).cpu().clone()
        o += n
    masks = tr.draw_masks(24, x.shape[1])
    want_loss, want_gn = lt.train_step(params, opt, x.cpu(), y.cpu(), masks={k: v.cpu() for k, v in masks.items()}, lengths=lens)
    loss = tr.train_step(x, y, masks, lengths=lens)
    assert np.isclose(float(loss.item()), want_loss, rtol=2e-5) and np.isclose(float(tr.gnorm.item()), want_gn, rtol=3e-4)


@pytest.mark.parametrize("H", [128, 64])
def test_train_step_with_dropout_masks_matches_oracle(tl, H):
    from evaluate_with_lstm import ConcentrationThresholdPredictor
    torch.manual_seed(H)
    B, T = 20, 10
    model = ConcentrationThresholdPredictor(hidden_size=H, device=DEV, seed=5)
    params = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    tr = tl.PredictorTrainer(model, lr=3e-4, seed=9)
    x = torch.rand(B, T, 1, device=DEV)
    y = torch.rand(B, device=DEV) * 50.0
    masks = tr.draw_masks(B, T)
    assert set(masks) == {"l0", "l1", "head"} and abs(float((masks["l0"] > 0).float().mean()) - 0.7) < 0.05
    opt = lt.AdamWState(params, lr=3e-4)
    cm = {k: v.cpu() for k, v in masks.items()}
    for k in range(2):
        want_loss, want_gn = lt.train_step(params, opt, x.cpu(), y.cpu(), masks=cm)
        loss = tr.train_step(x, y, masks)
        assert np.isclose(float(loss.item()), want_loss, rtol=2e-5)
        assert np.isclose(float(tr.gnorm.item()), want_gn, rtol=3e-4)
    for k, v in model.state_dict().items():
        assert torch.allclose(v.cpu(), params[k], rtol=2e-3, atol=3e-6), k


def test_training_run_fits_a_synthetic_relation(tl):
    """A few epochs of train_lstm() on synthetic plume trajectories whose source concentration is a simple function of
    the window: the epoch loss falls steadily (lr 3e-4 moves the output slowly, exactly as in the reference, which trains for
    150 epochs) and ReduceLROnPlateau follows torch's rule."""
    rng = np.random.RandomState(0)
    seqs, concs = [], []
    for i in range(256):
        L = int(rng.randint(12, 40))
        peak = 20.0 + 60.0 * rng.rand()
        s = peak / (1.0 + np.exp(-(np.arange(L) - L * 0.6) / 3.0)) + rng.rand(L)
        seqs.append(list(s))
        concs.append(float(peak))
    model, hist = tl.train_lstm(seqs, concs, epochs=12, device=DEV, seed=1, model_dir=None)
    assert np.isfinite(hist).all() and hist[-1] < hist[0] - 3.0 and hist[-1] <= min(hist) + 1e-9 + 0.2, hist
    sch = tl.ReduceLROnPlateau(3e-4)
    ora = lt.ReduceLROnPlateauOracle(3e-4)
    for m_ in [5, 4, 3, 3, 3, 3, 3, 3, 3, 3, 2.9999, 2.9999, 2.9999, 2.9999, 2.9999, 2.9999, 2.9999, 1.0]:
        assert sch.step(m_) == ora.step(m_)


# ---- V2.1 variant (PPOV2.1/train_lstm.py)
GOLD21 = os.path.join(os.path.dirname(__file__), "golden", "train_lstm_v21.npz")


def segments_of(g):
    return [{"positions": g["positions"][i], "concentrations": g["concentrations"][i], "source_pos": g["source_pos"][i]}
            for i in range(int(g["n_seg"]))]


def test_trajectory_dataset_matches_reference_golden(tl):
    import random
    g = np.load(GOLD21, allow_pickle=False)
    ds = tl.TrajectoryDataset(segments_of(g), stop_radius=10, window_size=int(g["window"]), rng=random.Random(5))
    assert len(ds) == 60 and np.array_equal(np.stack(ds.features)[:, :, 0], g["X"]) and np.array_equal(ds.labels, g["labels"])
    f, l = ds[1]
    assert f.shape == (20, 1) and l.shape == (2,) and f.dtype == torch.float32


def test_peak_stop_three_steps_match_the_reference_golden(tl):
    from evaluate_with_lstm import PeakAndStopPredictor
    g = np.load(GOLD21, allow_pickle=False)
    model = PeakAndStopPredictor(device=DEV)
    model.load_state_dict({k[5:]: g[k] for k in g.files if k.startswith("init/")})
    tr = tl.PeakStopTrainer(model)
    x = torch.tensor(g["X"][:32], dtype=torch.float32, device=DEV)[:, :, None].contiguous()
    y = torch.tensor(g["labels"][:32], dtype=torch.float32, device=DEV)
    for k in range(3):
        loss = tr.train_step(x, y)
        assert np.isclose(float(loss.item()), g["losses"][k], rtol=2e-5), (k, float(loss.item()), g["losses"][k])
        assert np.isclose(float(tr.gnorm.item()), g["gnorms"][k], rtol=2e-4)
    for k, v in model.state_dict().items():
        assert np.allclose(v.cpu().numpy(), g["post/" + k], rtol=2e-3, atol=3e-6), k


def test_mse_bce_matches_torch_including_saturated_logits():
    from uavppo import ops
    torch.manual_seed(3)
    for n in (777, 1, 256, 257):                 # one block of 256 threads: a single element, a full pass, one element into the second
        sat = 4 if n >= 4 else 0
        out = torch.randn(n, 2, device=DEV) * 3
        out[:sat, 1] = torch.tensor([60.0, -60.0, 120.0, -120.0], device=DEV)[:sat]      # sigmoid saturates: BCELoss clamps log at -100
        tgt = torch.stack([torch.randn(n, device=DEV), (torch.rand(n, device=DEV) > 0.5).float()], 1)
        loss, dout = ops.mse_bce(out, tgt)
        o = out.detach().cpu().double().requires_grad_(True)
        want = torch.nn.functional.mse_loss(o[:, 0], tgt[:, 0].cpu().double()) + \
            torch.nn.functional.binary_cross_entropy(torch.sigmoid(o[:, 1]).float().double(), tgt[:, 1].cpu().double())
        assert np.isclose(float(loss.item()), float(want), rtol=1e-5), n
        gz = torch.autograd.grad(torch.nn.functional.mse_loss(o[:, 0], tgt[:, 0].cpu().double()) +
                                 torch.nn.functional.binary_cross_entropy_with_logits(o[:, 1], tgt[:, 1].cpu().double()), o)[0]
        assert torch.allclose(dout.cpu().double()[sat:], gz[sat:], rtol=1e-4, atol=1e-8), n
    # a NaN in either column reaches the loss and that element's gradient (nn.BCELoss refuses a NaN probability outright;
    # a clamp that swallowed it would leave the loss finite); the other gradients keep their bits
    for col in (0, 1):
        bad = out.clone()
        bad[n - 1, col] = float("nan")
        loss2, dout2 = ops.mse_bce(bad, tgt)
        assert torch.isnan(loss2).all() and torch.isnan(dout2[n - 1, col])
        keep = torch.ones(n, 2, dtype=torch.bool, device=DEV)
        keep[n - 1, col] = False
        assert torch.equal(dout2[keep], dout[keep])


def test_train_peak_and_stop_learns_the_stop_label(tl, tmp_path):
    """Separable toy data: stop = 1 exactly when the window's last concentration is high.  Loss must fall and the
    saved best checkpoint must load back into the evaluation-side predictor."""
    import random
    from evaluate_with_lstm import PeakAndStopPredictor
    rng = np.random.RandomState(0)
    segs = []
    for e in range(96):
        src = rng.rand(2) * 100
        near = e % 2 == 0
        conc = np.linspace(1.0, 95.0 if near else 25.0, 32) + rng.rand(32)       # first window low, last window high iff near
        pos = np.tile(src + (2.0 if near else 30.0), (32, 1))
        segs.append({"positions": pos, "concentrations": conc, "source_pos": src, "sigma": 15.0})
    random.seed(1)
    model, hist = tl.train_peak_and_stop(segs, epochs=120, batch_size=64, device=DEV, seed=2, model_dir=str(tmp_path))
    assert hist[-1] < 0.5 * hist[0]
    m2 = PeakAndStopPredictor(device=DEV)
    m2.load_state_dict(torch.load(os.path.join(str(tmp_path), "best_peak_and_stop.pth")))
    x = torch.tensor(np.stack([s["concentrations"][-20:] for s in segs]) / 100.0, dtype=torch.float32, device=DEV)
    peak, stop = m2(x)
    assert float(stop[0::2].mean()) > float(stop[1::2].mean()) + 0.3
    assert abs(float(peak[0::2].mean()) - 0.955) < 0.15                           # the peak head regresses the last concentration / 100
