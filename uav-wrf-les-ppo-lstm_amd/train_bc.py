# train_bc.py -- behaviour cloning of expert (state, action) pairs on MI355X.
#
# The reference has no counterpart: its expert data (PPOV1.1/generate_expert_data.py) feed the GAIL discriminator only.  This
# script trains a policy to reproduce the expert's actions (uavppo.bc.BCTrainer on the fused cloning kernels) and saves it with
# the keys train_ppo2.0.py's _save writes, so evaluate_with_lstm.py, evaluate_model.py, generate_expert_data.load_policy and
# train_ppo_gail(init_model=...) load it unchanged.  An LSTM policy needs expert data written with lengths=True
# (generate_expert_data(..., lengths=True)): whole episodes are the unit it trains on.
import csv
import os

import numpy as np
import torch

from config import BC_BATCH, BC_EPOCHS, BC_LR, BC_VALUE_COEF, HIDDEN, NUM_LAYERS, SEED
from uavppo.bc import BCTrainer
from uavppo.policy import LSTMActorCritic, MLPActorCritic

METRIC_COLUMNS = ("epoch", "nll", "value_loss", "entropy", "accuracy", "samples")


def train_bc(expert_path="expert_data.npz", policy="mlp", hidden=HIDDEN, layers=NUM_LAYERS, epochs=BC_EPOCHS, batch=BC_BATCH,
             out="bc_model.pth", lr=BC_LR, value_coef=BC_VALUE_COEF, ent_beta=0.0, value_targets=None, seed=SEED, device="cuda",
             metrics_path="bc_metrics.csv"):
    """Clone the expert set at expert_path into a fresh policy ("mlp": the reference's 256-128 network, "lstm": the LSTM
    actor-critic with `hidden` x `layers`), `epochs` passes in chunks of `batch` (rows for the MLP, episodes for the LSTM); the
    observation width is the expert states'.  Writes the checkpoint `out` and one row per epoch to metrics_path (either may be
    None); prints a progress line per epoch.  Returns the trainer."""
    obs_dim = int(np.load(expert_path)["states"].shape[1])
    if policy == "lstm":
        pol = LSTMActorCritic(obs_dim, hidden, layers, 5, device, seed=seed)
    elif policy == "mlp":
        pol = MLPActorCritic(obs_dim, 5, device=device, seed=seed)
    else:
        raise ValueError(f"train_bc: policy={policy!r} ('mlp' or 'lstm')")
    tr = BCTrainer(pol, expert_path, batch=batch, lr=lr, value_coef=value_coef, ent_beta=ent_beta, seed=seed, value_targets=value_targets)
    rows = []
    for e in range(int(epochs)):
        tr.epoch()
        m = tr.metrics()
        rows.append([e + 1] + [m[k] for k in METRIC_COLUMNS[1:]])
        print(f"Epoch {e + 1} | NLL: {m['nll']:.4f} | Accuracy: {m['accuracy']:.2%} | Entropy: {m['entropy']:.4f}")
    if out:
        os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
        torch.save({k: v.cpu() for k, v in pol.state_dict().items()}, out)
    if metrics_path:
        with open(metrics_path, "w", newline="") as f:
            w = csv.writer(f, lineterminator="\n")
            w.writerow(METRIC_COLUMNS)
            w.writerows(rows)
    print(f"behaviour cloning finished: {int(epochs)} epochs, {tr.opt_step} optimiser steps; policy saved as {out}")
    return tr


def _main(argv):
    import argparse
    ap = argparse.ArgumentParser(description="behaviour cloning of expert_data.npz")
    ap.add_argument("--expert", default="expert_data.npz")
    ap.add_argument("--policy", default="mlp", choices=("mlp", "lstm"))
    ap.add_argument("--hidden", type=int, default=HIDDEN)
    ap.add_argument("--layers", type=int, default=NUM_LAYERS)
    ap.add_argument("--epochs", type=int, default=BC_EPOCHS)
    ap.add_argument("--batch", type=int, default=BC_BATCH)
    ap.add_argument("--out", default="bc_model.pth")
    a = ap.parse_args(argv)
    train_bc(a.expert, a.policy, a.hidden, a.layers, a.epochs, a.batch, a.out)


if __name__ == "__main__":
    import sys
    os.environ["KMP_DUPLICATE_LIB_OK"] = "TRUE"
    _main(sys.argv[1:])
