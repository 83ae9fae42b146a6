"""In-training greedy evaluation with a device-kept best model (VecPPOTrainer(eval_every=...)).

Every `eval_every` iterations the trainer's policy runs one greedy episode per env of a SEPARATE VecMethaneEnv, the env
evaluate() (evaluate_with_lstm.py) would be given: a fixed radius, never touched by the curriculum, reset before each evaluation
-- env_reset sets episode = 0, so every evaluation runs the same sources and the same wind noise (common random numbers).  The
bookkeeping of evaluate()'s _Episodes is three kernels (csrc/eval_track.hip), none of which the host waits for:

  uav_greedy_reduce    per chunk of records: which episodes ended, at which step, where, and whether by the stop rule
  uav_greedy_summary   per evaluation: steps / deviation / success per env and eight sums in one fixed order of summation
  uav_keep_best        best[:] = policy.flat[:] where the (all-reduced) sums beat the best evaluation so far

reduce_chunk, summarise and better_rule state them in numpy: what the kernels are tested against bit for bit, and what a log
reader replays a run with.  The rule: a row holding a NaN, with a NaN-logit count above 0 or without episodes is skipped; the first
valid row is better; later rows are better iff successes are strictly greater, or equal with a strictly smaller step sum; a tie
keeps the earlier model.

EvalTracker.run() issues launches and one non-blocking copy only; curve() returns the rows that have landed.  What is NOT in
here: the learned stop controllers inside the evaluation (the estimator's own rule is: source_stop=), a side stream, an early exit once every episode has ended (the number of chunks is
fixed at ceil(limit / chunk)).
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .greedy import GreedyRun, policy_core, policy_route
from .mirror_ring import MirrorRing
from .vec_env import VecMethaneEnv

SUM_N, BEST_N = ops.EVAL_SUM_N, ops.BEST_N
SLOTS = 256                  # threads of uav_greedy_summary's one block
CURVE_COLUMNS = ["Iteration", "Episodes", "Success_Rate", "Mean_Steps", "Mean_Deviation", "Std_Deviation", "Mean_Deviation_Success",
                 "Cut_Off", "Is_Best"]
CURVE_FILE = "eval_curve.csv"
BEST_MODEL_FILE = "best_model.pth"


def _int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def check_eval(eval_every=None, eval_envs=256, eval_seed=4321, eval_max_steps=None, eval_chunk=None, eval_radius=None,
               keep_best=True):
    """VecPPOTrainer's evaluation keywords, refused with the reason (ValueError); returns them as a dict of plain ints / floats /
    None.  Pure host arithmetic: the trainer calls it before it touches a device.  eval_every=None switches the evaluation off;
    the other keywords are still checked, so a typo does not wait for the day the option is turned on."""
    if eval_every is not None and not (_int(eval_every) and eval_every >= 1):
        raise ValueError(f"eval_every={eval_every!r}: a positive number of iterations, or None (no evaluation)")
    if not (_int(eval_envs) and 1 <= eval_envs <= 1 << 20):
        raise ValueError(f"eval_envs={eval_envs!r}: a number of evaluation envs between 1 and 2^20")
    if not (_int(eval_seed) and 0 <= eval_seed < 1 << 63):
        raise ValueError(f"eval_seed={eval_seed!r}: a non-negative integer")
    if eval_max_steps is not None and not (_int(eval_max_steps) and eval_max_steps >= 1):
        raise ValueError(f"eval_max_steps={eval_max_steps!r}: a positive number of steps, or None (the env's own limit)")
    if eval_chunk is not None and not (_int(eval_chunk) and eval_chunk >= 1):
        raise ValueError(f"eval_chunk={eval_chunk!r}: a positive number of steps per launch, or None")
    if eval_radius is not None:
        ok = isinstance(eval_radius, (int, float, np.integer, np.floating)) and not isinstance(eval_radius, bool)
        if not (ok and 0.0 < float(eval_radius) < float("inf")):
            raise ValueError(f"eval_radius={eval_radius!r}: a positive finite success radius, or None (the env's default)")
    if not isinstance(keep_best, (bool, np.bool_)):
        raise ValueError(f"keep_best={keep_best!r}: True or False")
    return dict(eval_every=None if eval_every is None else int(eval_every), eval_envs=int(eval_envs), eval_seed=int(eval_seed),
                eval_max_steps=None if eval_max_steps is None else int(eval_max_steps),
                eval_chunk=None if eval_chunk is None else int(eval_chunk),
                eval_radius=None if eval_radius is None else float(eval_radius), keep_best=bool(keep_best))


# ------------------------------------------------------------------------------------------ the numpy definitions
def fresh_episodes(n):
    """(ep_steps i32 [n], ep_state u8 [n], ep_pos f64 [n, 2]) of an evaluation that has not stepped yet: all zeros."""
    return np.zeros(n, np.int32), np.zeros(n, np.uint8), np.zeros((n, 2), np.float64)


def reduce_chunk(flags, obs, pos, t0, ep_steps, ep_state, ep_pos):
    """uav_greedy_reduce: new (ep_steps, ep_state, ep_pos) after one chunk of records flags u8 [n, k], obs f32 [n, k, D], pos f32
    [n, k, 2] that follows t0 steps.  ep_state bit0: ended, bit1: ended by the stop rule."""
    flags = np.asarray(flags, np.uint8)
    obs, pos = np.asarray(obs, np.float32), np.asarray(pos, np.float32)
    n, k = flags.shape
    ep_steps, ep_state, ep_pos = np.array(ep_steps, np.int32), np.array(ep_state, np.uint8), np.array(ep_pos, np.float64)
    for e in range(n):
        if ep_state[e] & 1:
            continue                                    # ended earlier: left alone
        first = -1
        for i in range(k):
            f = int(flags[e, i])
            if not f & 4 and f & 9:                     # bit2: not stepped, never an end; bit0 done, bit3 rule fired
                first = i
                break
        if first >= 0:
            f = int(flags[e, first])
            ep_steps[e] = t0 + first + 1
            ep_state[e] |= 1 | (2 if f & 8 else 0)
            if f & 1:                                   # the record holds the terminal observation
                ep_pos[e] = obs[e, first, :2].astype(np.float64) * 500.0
            else:
                ep_pos[e] = pos[e, first].astype(np.float64)
        elif not int(flags[e, k - 1]) & 4:              # still running: where a cut-off episode stands
            ep_pos[e] = pos[e, k - 1].astype(np.float64)
    return ep_steps, ep_state, ep_pos


def _tree(v):
    """wave_sum's tree over axis -2 (64 lanes -> lane 0), the kernel's shuffle-down order."""
    v = v.copy()
    o = 32
    while o > 0:
        v[..., :o, :] = v[..., :o, :] + v[..., o:2 * o, :]
        o >>= 1
    return v[..., 0, :]


def _block256(v):
    """block256_sum over axis -2 of [256, C]: the tree per wave of 64, then ((w0 + w1) + w2) + w3."""
    w = _tree(v.reshape(4, 64, v.shape[-1]))
    return ((w[0] + w[1]) + w[2]) + w[3]


def summarise(ep_steps, ep_state, ep_pos, src, limit, success_distance, nan_count=0):
    """uav_greedy_summary: dict(steps i32 [n], deviation f64 [n], success bool [n], stopped_early bool [n], sums f64 [8]) -- what
    _Episodes.metrics computes, and sums = {episodes, successes, sum of steps, of deviations, of squared deviations, of the
    successful episodes' deviations, episodes cut off by `limit`, nan_count}.  THE ORDER OF SUMMATION: slot j of 256 adds the
    envs j, j + 256, j + 512, ... one after the other; the 256 slots are added by block256_sum's tree.  A NaN position gives a
    NaN deviation, no success, and NaN in the sums it enters."""
    ep_steps, ep_state = np.asarray(ep_steps, np.int32), np.asarray(ep_state, np.uint8)
    ep_pos, src = np.asarray(ep_pos, np.float64), np.asarray(src, np.float64)
    n = ep_steps.shape[0]
    ended = (ep_state & 1) != 0
    steps = np.where(ended, ep_steps, np.int32(limit)).astype(np.int32)
    dx, dy = ep_pos[:, 0] - src[:, 0], ep_pos[:, 1] - src[:, 1]
    with np.errstate(invalid="ignore"):
        dev = np.sqrt(dx * dx + dy * dy)
        ok = dev <= np.float64(success_distance)
    vals = np.stack([ok.astype(np.float64), steps.astype(np.float64), dev, dev * dev, np.where(ok, dev, 0.0),
                     (~ended).astype(np.float64)], axis=1)
    acc = np.zeros((SLOTS, 6), np.float64)
    for r0 in range(0, n, SLOTS):
        c = vals[r0:r0 + SLOTS]
        acc[:c.shape[0]] += c
    sums = np.concatenate([[np.float64(n)], _block256(acc), [np.float64(nan_count)]])
    return {"steps": steps, "deviation": dev, "success": ok, "stopped_early": (ep_state & 2) != 0, "sums": sums}


def better_rule(state, sums, iteration):
    """uav_keep_best's decision: the new state f64 [7] = {best successes, best step sum, best iteration, evaluations seen,
    improvements, skipped, took} after the row `sums` of evaluation `iteration`; took = 1.0 iff the row became the best (and the
    kernel copied the parameters).  All zeros is the fresh state."""
    st = np.array(state, np.float64).reshape(BEST_N).copy()
    S = np.asarray(sums, np.float64).reshape(SUM_N)
    valid = bool(S[0] > 0.0) and not bool(S[7] > 0.0) and not bool(np.isnan(S).any())
    took = 0.0
    st[3] = st[3] + 1.0
    if not valid:
        st[5] = st[5] + 1.0
    elif st[4] == 0.0 or S[1] > st[0] or (S[1] == st[0] and S[2] < st[1]):
        st[0], st[1], st[2] = S[1], S[2], np.float64(iteration)
        st[4] = st[4] + 1.0
        took = 1.0
    st[6] = took
    return st


def curve_row(iteration, sums, state, source=None, stopped=None):
    """One eval_curve.csv row (CURVE_COLUMNS) from an evaluation's sums and the state behind it: plain python numbers.  source: the
    twelve sums of uav_source_summary or None -> source_fit.SOURCE_COLUMNS behind them (the sixteen of uav_source_summary6: those
    and source_aniso.SOURCE_COLUMNS6); stopped: the number of episodes the
    estimator's stop rule ended or None -> source_stop.STOP_COLUMN (their share of the episodes) behind those."""
    if stopped is not None:
        n = float(np.asarray(sums, np.float64)[0])
        return curve_row(iteration, sums, state, source) + [float(stopped) / n if n > 0 else float("nan")]
    if source is not None:
        from .source_aniso import SUM_N as SRC6_SUM_N, source_row6
        from .source_fit import source_row
        return curve_row(iteration, sums, state) + (source_row6 if len(source) == SRC6_SUM_N else source_row)(source)
    S = np.asarray(sums, np.float64)
    n, ok = float(S[0]), float(S[1])
    mean = float(S[3] / n) if n > 0 else float("nan")
    var = float(S[4] / n) - mean * mean if n > 0 else float("nan")
    std = float(np.sqrt(max(var, 0.0))) if var == var else float("nan")
    return [int(iteration), int(n), ok / n if n > 0 else float("nan"), float(S[2] / n) if n > 0 else float("nan"), mean, std,
            float(S[5] / ok) if ok > 0 else float("nan"), int(S[6]) if S[6] == S[6] else 0, int(np.asarray(state)[6] == 1.0)]


def curve_columns(source=False, stop=False, aniso=False):
    """eval_curve.csv's header: CURVE_COLUMNS, source_fit.SOURCE_COLUMNS behind them where the source estimate is on (and
    source_aniso.SOURCE_COLUMNS6 behind those for the six-term model), and source_stop.STOP_COLUMN behind those where the estimator
    also stops the episodes."""
    from .source_aniso import SOURCE_COLUMNS6
    from .source_fit import SOURCE_COLUMNS
    from .source_stop import STOP_COLUMN
    return (CURVE_COLUMNS + (SOURCE_COLUMNS if source or stop or aniso else []) + (SOURCE_COLUMNS6 if aniso else [])
            + ([STOP_COLUMN] if stop else []))


def write_curve(path, rows):
    """eval_curve.csv: curve_row of every landed evaluation (EvalTracker.curve()), NaN written as "nan"."""
    import csv
    with open(path, "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(curve_columns(any("source" in r for r in rows), any("stopped" in r for r in rows),
                                 any(len(r.get("source", ())) == 16 for r in rows)))
        w.writerows(curve_row(r["iteration"], r["sums"], r["state"], r.get("source"), r.get("stopped")) for r in rows)


class CurveLog:
    """eval_curve.csv of a training script, written as the rows land (one evaluation late, like the episode rows): add() after an
    iteration writes what has landed since, close() waits for the rest.  path None (ranks other than 0): nothing is written."""

    def __init__(self, path, source=False, stop=False, aniso=False):
        import csv
        self.n, self.f, self.w = 0, None, None
        if path:
            self.f = open(path, "w", newline="")
            self.w = csv.writer(self.f, lineterminator="\n")
            self.w.writerow(curve_columns(source, stop, aniso))

    def add(self, tracker, wait=False):
        rows = tracker.curve(wait)
        if self.w is not None:
            self.w.writerows(curve_row(r["iteration"], r["sums"], r["state"], r.get("source"), r.get("stopped")) for r in rows[self.n:])
        self.n = len(rows)

    def close(self, tracker):
        self.add(tracker, wait=True)
        if self.f is not None:
            self.f.close()


def save_best_model(tracker, model_path):
    """best_model.pth beside the saved model, with the model's own keys; returns the path."""
    import os
    path = best_model_path(model_path)
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    torch.save({k: v.cpu() for k, v in tracker.best_state_dict().items()}, path)
    return path


def curve_path(csv_path):
    """eval_curve.csv beside the episode CSV"""
    import os
    return os.path.join(os.path.dirname(csv_path) or ".", CURVE_FILE)


def best_model_path(model_path):
    """best_model.pth beside the saved model"""
    import os
    return os.path.join(os.path.dirname(model_path) or ".", BEST_MODEL_FILE)


# ------------------------------------------------------------------------------------------ the tracker
class EvalTracker:
    """The trainer's collaborator for eval_every (like LrController): owns the evaluation env, one GreedyRun on the route
    policy_route gives the policy, the episodes' device state, the rule's state and the best parameters so far.

    policy: the trainer's policy object (its flat is read, never written); kind "lstm" | "mlp".  rank / world shard the global env
    indices like the trainer's envs; collectives: the eight sums are all-reduced (dist_utils.allreduce_sum) before the rule, so
    every rank keeps the same model.  guard: the trainer's RangeGuard or None: once its lagged mirror says the parameters left the
    fp16-split range (guard.arith != "fp16x3", never a fresh read) an LSTM's later evaluations run on the tail route; until then an
    out-of-range evaluation on the fused kernels shows as sums[7] > 0 and is skipped by the rule.  An MLP has no tail route: its
    later evaluations are not run and are counted in `dropped`.  source_fit: None, True or a dict of check_source_fit's keywords
    (source_fit.py): one uav_source_moments per chunk in front of its uav_greedy_reduce, uav_source_solve and uav_source_summary
    behind uav_greedy_summary; the twelve sums ride in the mirrored row and are all-reduced with the eight.  No host read is
    added and the keep-best rule does not see them.  source_fit={"model": "aniso"}: the six-term kernels (source_aniso.py) and
    their SIXTEEN sums instead; bank_truth f64 [F, 4] = {sigma_major, sigma_minor, theta, peak} per field of `bank`, or None: each
    evaluation gathers its envs' rows on the device (env_core.h's field rule) for the summary's truth sums.  Not with source_stop.  source_stop: None, True or a dict of check_source_stop's keywords
    (source_stop.py; implies source_fit): one uav_source_stop_scan per chunk in front of the moments, which writes the estimator's
    stop into the records' flags and clears the greedy kernel's `active` there, so the bookkeeping and the estimate see the episode
    end where the rule said; one more value rides behind the twelve, the number of episodes the rule ended.  Give the evaluation
    env a small eval_radius where the rule is to do the stopping: its own success radius still ends episodes."""

    RING = 8            # evaluations whose rows may be on their way to the host at once

    def __init__(self, policy, kind, num_envs=256, variant="v2.0", trend_k=0, seed=4321, bank=None, bank_sources=None, device="cuda",
                 rank=0, world=1, max_steps=None, chunk=None, success_distance=40.0, keep_best=True, eval_radius=None, guard=None,
                 collectives=False, source_fit=None, source_stop=None, bank_truth=None):
        from .source_aniso import SUM_N as SRC6_SUM_N
        from .source_fit import SUM_N as SRC_SUM_N, SourceFit, is_aniso, option, variant_truth
        from .source_stop import SourceStop, option as stop_option
        c = check_eval(1, num_envs, seed, max_steps, chunk, eval_radius, keep_best)
        fit_cfg, stop_cfg = option(source_fit), stop_option(source_stop)
        if stop_cfg is not None and fit_cfg is None:
            fit_cfg = option(True)
        self.aniso = is_aniso(fit_cfg)
        if self.aniso and stop_cfg is not None:
            raise ValueError("EvalTracker(source_stop=...): not with source_fit model \"aniso\": the stop scan solves the four-term "
                             "system per record; a six-term scan does not exist")
        if bank_truth is not None and not self.aniso:
            raise ValueError("EvalTracker(bank_truth=...): only the six-term estimator (source_fit={\"model\": \"aniso\"}) scores "
                             "against it")
        self.policy, self.kind, self.guard, self.collectives = policy, kind, guard, bool(collectives)
        self.N, self.device = c["eval_envs"], torch.device(device)
        self.success_distance, self.keep = float(success_distance), c["keep_best"]
        self.env_args = dict(num_envs=self.N, variant=variant, device=self.device, seed=c["eval_seed"], bank=bank,
                             bank_sources=bank_sources, env_offset=int(rank) * self.N, n_env_total=int(world) * self.N, trend_k=int(trend_k))
        self.env = VecMethaneEnv(**self.env_args)
        if c["eval_radius"] is not None:
            self.env.current_radius = c["eval_radius"]
        self.limit = c["eval_max_steps"] or self.env.max_steps
        self.chunk = min(c["eval_chunk"] or 250, self.limit)
        if policy_core(policy) is None:
            raise TypeError("EvalTracker: expected the trainer's policy object")
        self.route = policy_route(policy, self.env, who="EvalTracker")
        if self.route == "stepwise":
            raise RuntimeError(f"EvalTracker: neither the fused greedy kernels nor the tail route cover this policy "
                               f"({type(policy).__name__}); the in-training evaluation has no step-wise path")
        self.greedy = GreedyRun(kind, policy, self.env, tail=self.route == "tail")
        self.dropped = 0             # evaluations not run: an MLP whose parameters left the fused kernels' range
        N, d = self.N, self.device
        # the episodes' state as ONE blob (one zeroing launch per evaluation): ep_pos f64 [N, 2] | ep_steps i32 [N] | ep_state u8 [N]
        self._blob = torch.zeros(21 * N, dtype=torch.uint8, device=d)
        self.ep_pos = self._blob[:16 * N].view(torch.float64).view(N, 2)
        self.ep_steps = self._blob[16 * N:20 * N].view(torch.int32)
        self.ep_state = self._blob[20 * N:]
        self.src = torch.zeros(N, 2, dtype=torch.float64, device=d)
        self.deviation = torch.zeros(N, dtype=torch.float64, device=d)
        self.steps = torch.zeros(N, dtype=torch.int32, device=d)
        self.success = torch.zeros(N, dtype=torch.uint8, device=d)
        # [sums | source sums | stopped | state]: what the ring mirrors; the sums stand together, so one all-reduce takes them all
        self.n_src = (SRC6_SUM_N if self.aniso else SRC_SUM_N) if fit_cfg is not None else 0
        self.n_stop = 1 if stop_cfg is not None else 0
        self.n_extra = self.n_src + self.n_stop
        self.row = torch.zeros(SUM_N + self.n_extra + BEST_N, dtype=torch.float64, device=d)
        self.sums, self.state = self.row[:SUM_N], self.row[SUM_N + self.n_extra:]
        self.fit = None          # source_fit.SourceFit: where the records say the source is, beside the bookkeeping
        if fit_cfg is not None:
            self.fit = SourceFit(N, d, **fit_cfg)
            self.src_sums = self.row[SUM_N:SUM_N + self.n_src]
            self.truth = variant_truth(variant) if bank is None else (float("nan"), float("nan"))
            # model "aniso": f64 [F, 4] per field of the bank, or None; each evaluation gathers its envs' rows on the device
            self.bank_truth = None if bank_truth is None else torch.as_tensor(bank_truth, dtype=torch.float64).to(d)
            if self.bank_truth is not None:
                from .source_aniso import gather_truth
                gather_truth(self.bank_truth, self.env)          # the shape check, once
        self.stop = None         # source_stop.SourceStop: the estimator as the stop rule, in front of the moments
        if stop_cfg is not None:
            self.stop = SourceStop(N, d, fit_cfg=fit_cfg, **stop_cfg)
            self.stopped = self.row[SUM_N + self.n_src:SUM_N + self.n_extra]
        self.best = torch.zeros_like(policy.flat)
        self.ring = MirrorRing((self.row.numel(),), torch.float64, slots=self.RING)
        self._iters = []             # iteration of every slot in flight, oldest first
        self._rows = []              # landed rows

    def _run_for_now(self):
        """The GreedyRun of this evaluation, or None (dropped).  Reads the guard's lagged decision only."""
        if self.route == "fused" and self.guard is not None and self.guard.enabled and self.guard.arith != "fp16x3":
            if self.kind != "lstm":
                return None
            self.route = "tail"       # once per run: builds the tail backend (its constructor measures max |param| once)
            self.greedy = GreedyRun(self.kind, self.policy, self.env, tail=True)
        return self.greedy

    def run(self, iteration):
        """One evaluation of the policy's current parameters, tagged `iteration`: env.reset(), ceil(limit / chunk) times (a chunk
        of greedy steps, uav_greedy_reduce), uav_greedy_summary, the all-reduce of the sums where collectives are on,
        uav_keep_best on policy.flat, and the row [sums | state] pushed towards the host.  The number of launches is fixed; the
        host reads nothing.  (Only when the ring is full -- the host is RING evaluations ahead of the device -- does it wait for
        the oldest row.)"""
        greedy = self._run_for_now()
        if greedy is None:
            self.dropped += 1
            return
        env, N = self.env, self.N
        env.reset()
        ops.env_peek(env.state, N, source=self.src)
        truth6 = None
        if self.aniso:                                       # the truth of the episodes whose sources were just taken
            from .source_aniso import gather_truth
            truth6 = gather_truth(self.bank_truth, env)
        greedy.restart()
        self._blob.zero_()
        if self.fit is not None:
            self.fit.restart()
        if self.stop is not None:
            self.stop.restart()
        t0 = 0
        while t0 < self.limit:
            k = min(self.chunk, self.limit - t0)
            recs = greedy.chunk(t0, k)
            if self.stop is not None:                        # marks its hits in recs["flags"], clears greedy.active there
                self.stop.scan(recs, t0, self.ep_state, greedy.active)
            if self.fit is not None:
                self.fit.chunk(recs, self.ep_state)          # ep_state as it stands before this chunk's reduce
            ops.greedy_reduce(recs, t0, self.ep_steps, self.ep_state, self.ep_pos)
            t0 += k
        ops.greedy_summary(self.ep_steps, self.ep_state, self.ep_pos, self.src, self.limit, self.success_distance, self.sums,
                           nan_count=greedy.nan_count, deviation=self.deviation, steps=self.steps, success=self.success)
        if self.fit is not None:
            self.fit.finish(self.src, *self.truth, truth=truth6, sums=self.src_sums)
        if self.stop is not None:                            # ep_state bit1, summed: the episodes the rule ended
            torch.sum((self.ep_state & 2).view(N, 1), dim=0, dtype=torch.float64, out=self.stopped)
            self.stopped.mul_(0.5)
        if self.collectives:
            from .dist_utils import allreduce_sum
            allreduce_sum(self.row[:SUM_N + self.n_extra])
        if self.keep:
            ops.keep_best(self.state, self.sums, iteration, self.policy.flat, self.best)
        if len(self.ring) == self.ring.slots:
            self.ring.wait(self.ring.oldest)
            self._collect_landed()
        self.ring.push(self.row)
        self._iters.append(int(iteration))

    def _collect_landed(self):
        ring = self.ring
        while ring.in_flight and ring.events[ring.in_flight[0]].query():
            k = ring.in_flight.pop(0)
            row = ring.host[k].numpy().copy()
            r = {"iteration": self._iters.pop(0), "sums": row[:SUM_N], "state": row[SUM_N + self.n_extra:]}
            if self.n_src:
                r["source"] = row[SUM_N:SUM_N + self.n_src]
            if self.n_stop:
                r["stopped"] = float(row[SUM_N + self.n_src])
            self._rows.append(r)

    def curve(self, wait=False):
        """The evaluations whose rows have landed, oldest first: dicts of iteration, sums f64 [8], state f64 [7] (after that
        evaluation's decision; state[6] == 1: it became the best), and with source_fit on source f64 [12], uav_source_summary's
        sums (model "aniso": f64 [16], uav_source_summary6's), and with source_stop on stopped, the number of episodes the estimator's rule ended.  wait=True waits for every
        evaluation issued so far."""
        if wait:
            for k in list(self.ring.in_flight):
                self.ring.events[k].synchronize()
        self._collect_landed()
        return list(self._rows)

    def best_flat(self):
        """A copy of the best parameters so far (zeros before the first valid evaluation).  Waits for the device."""
        torch.cuda.current_stream(self.device).synchronize()
        return self.best.clone()

    def best_state_dict(self):
        """The best parameters under the policy's own state_dict keys (with normalise_obs: the folded, deployable ones).  Waits."""
        flat, best = self.policy.flat, self.best_flat()
        out = {}
        for k, v in self.policy.named_views().items():
            o = v.storage_offset() - flat.storage_offset()
            out[k] = best[o:o + v.numel()].view(v.shape).clone()
        return out

