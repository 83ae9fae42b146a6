"""evaluate_model.py -- greedy evaluation with the "autonomous stop" rule on the MI355X path.

Counterpart of the reference's PPOV1.1/evaluate_model.py (ModelEvaluator, :10-90), vectorised: its `eval_episodes`
sequential episodes of a V1.1 MethaneEnv become that many parallel environments of a VecMethaneEnv(..., "v1.1") with one
episode each.  Same class and attribute names, the same CSV (evaluation_results.csv: episode, steps, deviation, success,
final_conc) and the same stop rule (:25-37): once 10 positions are recorded, stop when np.std of the last 10 agent
positions, averaged over the two coordinates, is below 2.0 px AND the step's concentration is above the threshold.

The rule runs on the device.  Where the fused greedy-episode kernels cover the policy (uavppo.greedy.fused_refusal:
the reference's MLP or one LSTM layer of h = 64 / 128, fp16-split arithmetic, parameters in range) whole chunks of steps are
one launch each of uav_greedy_episodes_stop -- the env lane pushes agent_pos into its window, evaluates the rule and freezes
the env on a hit -- and the host only reduces the records: an env's episode ends at its first record with flags bit0 (done)
or bit3 (stopped by the rule).  Every other LSTM policy (stacked layers, h = 256, parameters out of range: uavppo.greedy.tail_refusal)
runs the same chunks on the tail route: per env step the layers' step kernels and one uav_greedy_tail launch, which applies the rule
as the fused kernels do.  What is left steps one launch sequence per time step, with the rule applied by uav_stop_stability (the same
device function).  No CPU fallback: everything goes through uavppo.ops.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from config import CONC_PEAK, CONC_REWARD_COEF
from uavppo import ops
from uavppo.greedy import GreedyRun, fused_refusal, policy_core, policy_route, stepwise_policy_probs  # noqa: F401  (fused_refusal: tests)
from uavppo.source_aniso import gather_truth
from uavppo.source_fit import ESTIMATE_FILE, SourceFit, is_aniso, variant_truth, write_estimates
from uavppo.source_fit import option as source_fit_option

F32 = torch.float32
CSV_COLUMNS = ("episode", "steps", "deviation", "success", "final_conc")
DONE, STOPPED = 1, 8                  # bits of a record's flags (include/uavppo.h)


def write_results_csv(path, steps, deviations, success, final_conc):
    """evaluation_results.csv as the reference's `pd.DataFrame(results).to_csv(path, index=False)` writes it (:86-87): int64
    episode (from 1) and steps, float64 deviation and float32 final_conc in their shortest round-trip form, bool success."""
    with open(path, "w", newline="") as f:
        f.write(",".join(CSV_COLUMNS) + "\n")
        for i in range(len(steps)):
            f.write(f"{i + 1},{int(steps[i])},{float(np.float64(deviations[i]))!r},{bool(success[i])},"
                    f"{np.float32(final_conc[i])!s}\n")


class ModelEvaluator:
    """model_path_or_policy: a reference-keyed .pth of PPOActorCritic(6, 5) (as the reference), or a policy object
    (LSTMActorCritic, MLPActorCritic, model.PPOActorCritic).  env: a VecMethaneEnv of `eval_episodes` environments (default:
    v1.1, procedural fields, radius 50 -- the reference builds a fresh MethaneEnv, no curriculum).  run_evaluation() takes the
    fused greedy kernels where they cover the policy, the tail route (the LSTM layers' step kernels + uav_greedy_tail per env step)
    for every other LSTMActorCritic, and the step-wise loop for what is left; its fused= / tail= keywords force a route."""

    def __init__(self, model_path_or_policy, eval_episodes=1000, device="cuda", env=None):
        from uavppo.vec_env import VecMethaneEnv
        self.device = torch.device(device)
        self.eval_episodes = int(eval_episodes)
        if env is not None and env.num_envs != self.eval_episodes:
            raise ValueError(f"ModelEvaluator: env has {env.num_envs} environments, eval_episodes = {self.eval_episodes}")
        self.env = env if env is not None else VecMethaneEnv(self.eval_episodes, "v1.1", self.device)
        self.model = (self._load_model(model_path_or_policy) if isinstance(model_path_or_policy, (str, bytes)) or
                      hasattr(model_path_or_policy, "__fspath__") else model_path_or_policy)
        _policy_core_checked(self.model)
        self.position_window = 10                  # window of the position-stability test
        self.stability_threshold = 2.0             # px
        self.conc_threshold = 0.8 * CONC_PEAK

    def _load_model(self, path):
        from model import PPOActorCritic
        sd = torch.load(path, map_location="cpu")
        model = PPOActorCritic(int(sd["feature.0.weight"].shape[1]), 5, device=self.device)      # 6, or 6 + trend_k
        model.load_state_dict(sd)
        model.eval()
        return model

    def _rule(self):
        return ops.make_stop_rule(self.position_window, self.stability_threshold, CONC_REWARD_COEF, CONC_PEAK, self.conc_threshold)

    @torch.no_grad()
    def run_evaluation(self, noise=None, max_steps=2000, fused=None, chunk=None, csv_path="evaluation_results.csv", tail=None,
                       source_fit=None, bank_truth=None):
        """One greedy episode per environment, all together, each until done, the stop rule, or `max_steps` (:52).
        noise: optional f64 [max_steps, N, 2] standard normals (parity tests).  fused: None = the fused kernels where
        fused_refusal allows, else step-wise; True = fused or a RuntimeError naming why not; False = step-wise.  tail: None = the
        tail route where the fused kernels refuse the policy and tail_refusal allows; True = the tail route or a RuntimeError naming
        why not; False = never (fused=False alone still means step-wise).  The tail route gives the step-wise loop's rows: where
        `done` ends an episode its position is read off the terminal observation, as there.  chunk: steps per fused launch or per
        host visit of the tail route (default 250).  csv_path: where the reference's CSV goes (None: not written).
        Returns numpy arrays of length N: steps, deviations (f64), success (deviation < current_radius), final_conc (f32,
        (CONC_REWARD_COEF * obs[2]) * CONC_PEAK of the last step) and stopped_early (the rule fired on the last step).
        A NaN logit raises RuntimeError("NaN in probs").
        source_fit: None (off), True or a dict of uavppo.source_fit.check_source_fit's keywords: where each episode's measurements
        say the source is (uav_source_moments per chunk of records -- the stop rule's bit3 ends an episode for it as `done` does --
        then uav_source_solve / uav_source_summary).  The result gains evaluate()'s source_* arrays and source_estimates.csv is
        written beside csv_path; evaluation_results.csv stays byte for byte.  Fused and tail routes only (ValueError otherwise).
        source_fit={"model": "aniso"}: the six-term fit (uavppo/source_aniso.py); source_estimates.csv then has Sigma_Minor and Theta
        columns behind Sigma (the major width); bank_truth f64 [F, 4] or None: the per-field truth, as evaluate() takes it."""
        kind, core = _policy_core_checked(self.model)
        env = self.env
        fit_cfg = source_fit_option(source_fit)
        route = policy_route(self.model, env, fused, tail, "run_evaluation")
        if route == "stepwise" and fit_cfg is not None:
            raise ValueError("run_evaluation(source_fit=...): the estimator reads the records of the fused and tail routes; the "
                             "step-wise route keeps none")
        if route == "stepwise" and chunk is not None:
            raise ValueError("run_evaluation(chunk=...): chunks belong to the fused path")
        env.reset()
        _, src, _, _ = env.peek()
        aniso = is_aniso(fit_cfg)
        if bank_truth is not None and not aniso:
            raise ValueError("run_evaluation(bank_truth=...): only the six-term estimator (source_fit={\"model\": \"aniso\"}) scores "
                             "against it")
        fit = SourceFit(env.num_envs, env.device, **fit_cfg) if fit_cfg is not None else None
        truth = gather_truth(bank_truth, env) if aniso else None
        src_dev = src.to(torch.float64).clone() if fit is not None else None
        src = src.cpu().numpy()
        if route != "stepwise":
            steps, pos, obs2, stopped = self._episodes_fused(kind, core, noise, int(max_steps), int(chunk or 250),
                                                             tail=route == "tail", fit=fit)
        else:
            steps, pos, obs2, stopped = self._episodes_stepwise(kind, core, noise, int(max_steps))
        pos, obs2 = pos.cpu().numpy().astype(np.float32), obs2.cpu().numpy().astype(np.float32)
        d = pos.astype(np.float64) - src                                            # f32 agent_pos - f64 source_pos (:41)
        deviations = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
        out = {"steps": steps.cpu().numpy(), "deviations": deviations, "success": deviations < env.current_radius,
               "final_conc": (np.float32(CONC_REWARD_COEF) * obs2) * np.float32(CONC_PEAK),
               "stopped_early": stopped.cpu().numpy()}
        if csv_path is not None:
            write_results_csv(csv_path, out["steps"], out["deviations"], out["success"], out["final_conc"])
        if fit is not None:
            fit.finish(src_dev, *(variant_truth(env.variant) if env.bank is None else (float("nan"), float("nan"))), truth=truth)
            out.update(fit.metrics())
            if csv_path is not None:
                write_estimates(os.path.join(os.path.dirname(csv_path) or ".", ESTIMATE_FILE), out)
        return out

    def _episodes_fused(self, kind, core, noise, limit, chunk, want=None, tail=False, fit=None):
        """Per env: steps, final agent_pos (f32), obs[2] of the last step, stopped-by-the-rule -- reduced from the records of
        uav_greedy_episodes_stop, or with tail=True of GreedyRun's tail backend; the position of a step that ended its episode
        by `done` is then obs[:2] * 500 of the terminal observation rounded to f32, as _episodes_stepwise takes it (within an
        ulp of agent_pos), so both give the same rows.  want: optional dict that receives the concatenated records and rule_val
        (tests)."""
        env = self.env
        N, dev = env.num_envs, env.device
        run = GreedyRun(kind, core, env, self._rule(), tail=tail)
        active = torch.ones(N, dtype=torch.bool, device=dev)
        steps = torch.zeros(N, dtype=torch.int64, device=dev)
        stopped = torch.zeros(N, dtype=torch.bool, device=dev)
        pos = torch.zeros(N, 2, dtype=F32, device=dev)
        obs2 = torch.zeros(N, dtype=F32, device=dev)
        rows = torch.arange(N, device=dev)
        kept = []
        t0 = 0
        while t0 < limit:
            k = min(chunk, limit - t0)
            rv = torch.empty(N, k, dtype=F32, device=dev) if want is not None else None
            recs = run.chunk(t0, k, noise, rule_val=rv)
            if fit is not None:                                        # before this chunk's ends are taken
                fit.chunk(recs, (~active).to(torch.uint8))
            if want is not None:
                kept.append(dict(recs, rule_val=rv))
            end_c = (recs["flags"] & (DONE | STOPPED)) != 0            # an episode ends at its first such record
            ended = active & end_c.any(1)
            last = torch.where(ended, end_c.to(torch.int32).argmax(1), torch.full_like(rows, k - 1))
            steps = torch.where(ended, last + (t0 + 1), steps)
            stopped |= ended & ((recs["flags"][rows, last] & STOPPED) != 0)
            # envs still running took every step of the chunk: their last record is the cap's, should this be the last chunk
            take = active
            p_last = recs["pos"][rows, last]
            if tail:
                p_last = torch.where(((recs["flags"][rows, last] & DONE) != 0)[:, None],
                                     (recs["obs"][rows, last, :2].to(torch.float64) * 500.0).to(F32), p_last)
            pos = torch.where(take[:, None], p_last, pos)
            obs2 = torch.where(take, recs["obs"][rows, last, 2], obs2)
            active = active & ~ended
            t0 += k
            if not bool(active.any()):
                break
        run.raise_on_nan()
        steps = torch.where(active, torch.full_like(steps, limit), steps)          # cut off by `max_steps`
        if want is not None:
            want.update({key: torch.cat([r[key] for r in kept], 1) for key in kept[0]})
            want.update(stop_win=run.stop_win, stop_cnt=run.stop_cnt, h=run.h, c=run.c, active=run.active)
        return steps, pos, obs2, stopped

    def _episodes_stepwise(self, kind, core, noise, limit, want=None):
        """The same per-env results, one launch sequence per step: policy heads, argmax, uav_env_step, uav_stop_stability.
        The env auto-resets on done, so the position of a step that ended the episode is taken from the terminal
        observation (obs[:2] * 500 rounded to f32: within an ulp of agent_pos); every other step's is agent_pos itself."""
        env = self.env
        N, dev = env.num_envs, env.device
        rule = self._rule()
        probs, nan = stepwise_policy_probs(kind, core, env)
        stop_win = torch.zeros(N, rule.window, 2, dtype=F32, device=dev)
        stop_cnt = torch.zeros(N, dtype=torch.int32, device=dev)
        active = torch.ones(N, dtype=torch.bool, device=dev)
        steps = torch.zeros(N, dtype=torch.int64, device=dev)
        stopped = torch.zeros(N, dtype=torch.bool, device=dev)
        pos = torch.zeros(N, 2, dtype=F32, device=dev)
        obs2 = torch.zeros(N, dtype=F32, device=dev)
        vals, o2s = ([], []) if want is not None else (None, None)
        obs = env.obs
        for t in range(1, limit + 1):
            act = torch.argmax(probs(obs), dim=1).to(torch.int32)
            obs, _, done, _ = env.step(act, None if noise is None else noise[t - 1])
            done_b = done > 0.5
            pos_now, _, _, _ = env.peek()
            p = torch.where(done_b[:, None], (env.term_obs[:, :2].to(torch.float64) * 500.0).to(F32), pos_now).contiguous()
            o2 = torch.where(done_b, env.term_obs[:, 2], obs[:, 2]).contiguous()
            hit, val = ops.stop_stability(rule, p, o2, stop_win, stop_cnt, active=active.to(torch.uint8))
            if vals is not None:
                vals.append(val.clone())
                o2s.append(o2)
            pos = torch.where(active[:, None], p, pos)
            obs2 = torch.where(active, o2, obs2)
            ended = active & (done_b | (hit != 0))
            steps = torch.where(ended, torch.full_like(steps, t), steps)
            stopped |= ended & (hit != 0)
            active = active & ~ended
            if t % 16 == 0 and not bool(active.any()):
                break
        if int(nan.item()) > 0:
            raise RuntimeError("NaN in probs")                                     # model.py:47-49
        steps = torch.where(active, torch.full_like(steps, limit), steps)
        if want is not None:
            want.update(rule_val=torch.stack(vals, 1), obs2=torch.stack(o2s, 1), stop_win=stop_win, stop_cnt=stop_cnt)
        return steps, pos, obs2, stopped


def _policy_core_checked(policy):
    pc = policy_core(policy)
    if pc is None:
        raise TypeError(f"ModelEvaluator: expected a model path, LSTMActorCritic, MLPActorCritic or PPOActorCritic, "
                        f"got {type(policy).__name__}")
    return pc


def main(num_envs=1000, model_path="model/ppo_successful_models.pth", device="cuda", policy="mlp"):
    """The reference's __main__ (:92-94): 1000 episodes of model/ppo_successful_models.pth.  policy="lstm": the vectorised
    trainer's LSTM actor-critic checkpoint under the same file name."""
    if policy not in ("mlp", "lstm"):
        raise ValueError(f"main: policy must be 'mlp' or 'lstm', got {policy!r}")
    try:
        if policy == "lstm":
            from evaluate_with_lstm import load_lstm_policy
            evaluator = ModelEvaluator(load_lstm_policy(model_path, device), eval_episodes=num_envs, device=device)
        else:
            evaluator = ModelEvaluator(model_path, eval_episodes=num_envs, device=device)
    except FileNotFoundError as e:
        print(f"model file missing: {e}")
        return None
    out = evaluator.run_evaluation()
    print(f"validation done: success rate {out['success'].mean():.2%}, mean deviation {out['deviations'].mean():.1f} px, "
          f"stopped by the rule {out['stopped_early'].mean():.2%}")
    return out


if __name__ == "__main__":
    import sys
    main(policy="lstm" if "--lstm" in sys.argv[1:] else "mlp")
