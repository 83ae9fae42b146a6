"""update_diagnostics.csv: one row per training iteration with the last run epoch's update diagnostics
(VecPPOTrainer.diagnostics()), written beside the per-episode CSV by the training scripts when config.PPO_DIAGNOSTICS
(or config.TARGET_KL) is set.  The per-episode CSV is not touched."""
from __future__ import annotations

import csv
import os

FILE_NAME = "update_diagnostics.csv"
VALUES = ("approx_kl", "approx_kl_k1", "clip_fraction", "value_clip_fraction", "explained_variance")
COLUMNS = ("Iteration", "Epochs_Run") + tuple(v.title() for v in VALUES)
SCHEDULE_COLUMNS = ("Learning_Rate", "Entropy_Beta")      # the values the iteration's update ran with, when a schedule is in force


def path_beside(csv_path):
    """update_diagnostics.csv in the directory of the episode CSV (None without one)."""
    return os.path.join(os.path.dirname(os.path.abspath(csv_path)), FILE_NAME) if csv_path else None


def last_epoch_row(iteration, diag):
    """[iteration, epochs_run, the five values of the last epoch that ran] from a diagnostics() dict."""
    return [int(iteration), int(diag["epochs_run"])] + [float(diag[v][-1]) for v in VALUES]


def progress_text(diag):
    """The same values for a progress line."""
    kl, k1, cf, vcf, ev = (diag[v][-1] for v in VALUES)
    return f"epochs {diag['epochs_run']} | kl {kl:.3e} (k1 {k1:.3e}) | clip {cf:.3f} vclip {vcf:.3f} | expl.var {ev:.3f}"


class UpdateDiagnosticsLog:
    """Rows are flushed as they come: a run that is interrupted keeps what it measured.  path None (a rank other than 0, or a run
    without a CSV) keeps the rows in memory only.  extra_columns: names of further columns behind COLUMNS (a run with a
    schedule: SCHEDULE_COLUMNS), whose values add() then takes; without them the file is what it has always been."""

    def __init__(self, path, extra_columns=()):
        self.path, self.rows = path, []
        self.extra_columns = tuple(extra_columns)
        self._f = self._w = None
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            self._f = open(path, "w", newline="")
            self._w = csv.writer(self._f, lineterminator="\n")
            self._w.writerow(COLUMNS + self.extra_columns)
            self._f.flush()

    def add(self, iteration, diag, extra=()):
        if len(extra) != len(self.extra_columns):
            raise ValueError(f"{len(extra)} extra values for the columns {self.extra_columns}")
        row = last_epoch_row(iteration, diag) + [float(v) for v in extra]
        self.rows.append(row)
        if self._w is not None:
            self._w.writerow(row)
            self._f.flush()
        return row

    def close(self):
        if self._f is not None:
            self._f.close()
            self._f = self._w = None
