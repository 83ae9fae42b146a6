# train_ppo_gail.py -- PPO + GAIL on MI355X.
#
# Counterpart of the reference's PPOV1.1/train_ppo_gail.py: a policy trained by PPO while a discriminator learns to tell the
# rollout's (state, action) pairs from an expert set (generate_expert_data.py), one discriminator step per policy update
# (:150-175).  Here the loop is uavppo.gail.GAILTrainer over NUM_ENVS vectorised environments, and the discriminator's output
# is USED: the rollout's reward is env_coef * r + gail_coef * softplus(z) (the reference computes the discriminator and feeds
# it to nothing).  The policy side is the project's _update_model path by default; --update-form inline_v10 --minibatch-rows B
# (MLP policy) runs the reference's own inline update of :71-148 -- bootstrapped GAE, returns from the raw advantage, shuffled
# row minibatches (uavppo/trainer.py).  Not carried over: the TensorBoard histograms.
import os

import numpy as np
import torch

from config import (BPTT_LEN, CLIP_EPSILON, ENTROPY_BETA, ENV_VARIANT, EPOCHS, GAE_MODE, GAMMA, HIDDEN, HORIZON, LAMBDA, LEARNING_RATE, NUM_ENVS,
                    NORMALISE_OBS, NORMALISE_REWARDS, NUM_LAYERS, NUM_MINIBATCHES, OBS_NORM_EPS, POLICY, PPO_DIAGNOSTICS, REWARD_CLIP, SEED, SHUFFLE_ENVS, TARGET_KL)
from config import DESIRED_KL, ENTROPY_BETA_FINAL, LR_FACTOR, LR_FINAL, LR_MAX, LR_MIN, LR_SCHEDULE, SCHEDULE_ITERATIONS
from config import EVAL_ENVS, EVAL_EVERY, EVAL_MAX_STEPS, EVAL_SEED, EVAL_SOURCE_FIT, EVAL_SOURCE_STOP, KEEP_BEST
from model import Discriminator, compute_discriminator_loss, get_expert_data  # noqa: F401  (train_ppo_gail.py:24-27)
from uavppo.gail import GAILTrainer


def train_ppo_gail(num_episodes=2000, num_envs=NUM_ENVS, horizon=HORIZON, expert_path="expert_data.npz", policy=POLICY,
                   hidden=HIDDEN, gail_coef=1.0, env_coef=1.0, disc_lr=LEARNING_RATE, disc_steps=1, seed=SEED, device="cuda",
                   model_path="ppo_gail_model.pth", disc_path="discriminator.pth", max_iterations=None, update_form="update_model",
                   minibatch_rows=None, init_model=None):
    """Run GAILTrainer until num_episodes episodes have finished (the reference trains 2000, train_ppo_gail.py:49) or
    max_iterations rollouts were collected; print the reference's progress line every 10 iterations (:201-203, its
    `episode` read as the iteration); save the policy as ppo_gail_model.pth (:208) and the discriminator as
    discriminator.pth.  init_model: the path of a policy checkpoint (train_bc.py's, train_ppo2.0.py's) loaded into the
    trainer's policy before the first rollout; None starts from the seeded initialisation.  Returns the trainer."""
    states, actions = get_expert_data(expert_path)
    tr = GAILTrainer(num_envs, horizon, policy, hidden=hidden, layers=NUM_LAYERS, variant=ENV_VARIANT, seed=seed, device=device,
                     gae_mode=GAE_MODE, num_minibatches=NUM_MINIBATCHES, shuffle_envs=SHUFFLE_ENVS, bptt_len=BPTT_LEN, gamma=GAMMA, lam=LAMBDA, clip=CLIP_EPSILON,
                     ent_beta=ENTROPY_BETA, lr=LEARNING_RATE, epochs=EPOCHS, expert=(states, actions), gail_coef=gail_coef,
                     env_coef=env_coef, disc_lr=disc_lr, disc_steps=disc_steps, update_form=update_form, minibatch_rows=minibatch_rows,
                     diagnostics=PPO_DIAGNOSTICS, target_kl=TARGET_KL, normalise_rewards=NORMALISE_REWARDS, reward_clip=REWARD_CLIP,
                     normalise_obs=NORMALISE_OBS, obs_norm_eps=OBS_NORM_EPS, lr_schedule=LR_SCHEDULE, lr_final=LR_FINAL,
                     ent_beta_final=ENTROPY_BETA_FINAL, schedule_iterations=SCHEDULE_ITERATIONS, desired_kl=DESIRED_KL, lr_factor=LR_FACTOR,
                     lr_min=LR_MIN, lr_max=LR_MAX, eval_every=EVAL_EVERY, eval_envs=EVAL_ENVS, eval_seed=EVAL_SEED,
                     eval_max_steps=EVAL_MAX_STEPS, keep_best=KEEP_BEST, eval_source_fit=EVAL_SOURCE_FIT, eval_source_stop=EVAL_SOURCE_STOP)
    if init_model is not None:
        tr.policy.load_state_dict(torch.load(init_model, map_location="cpu"))
    # config.EVAL_EVERY: eval_curve.csv beside the saved policy, one row per greedy evaluation (train_iteration() runs it), written one
    # evaluation late as the rows land; best_model.pth beside the policy at the end
    eval_log = None
    if tr.eval_tracker is not None:
        from uavppo.eval_track import CurveLog, curve_path, save_best_model
        eval_log = CurveLog(curve_path(model_path or "ppo_gail_model.pth"), source=tr.eval_tracker.fit is not None, stop=tr.eval_tracker.stop is not None)
    # config.PPO_DIAGNOSTICS (or TARGET_KL, or LR_SCHEDULE "adaptive"): update_diagnostics.csv beside the saved policy, one row per
    # iteration (one host wait each); with a schedule in force the row ends in the step size and entropy weight its update ran with
    diag_log = diag = None
    sched = ()
    if PPO_DIAGNOSTICS or TARGET_KL is not None or LR_SCHEDULE == "adaptive":
        from uavppo.update_log import SCHEDULE_COLUMNS, UpdateDiagnosticsLog, path_beside, progress_text
        scheduled = LR_SCHEDULE != "constant" or ENTROPY_BETA_FINAL is not None
        diag_log = UpdateDiagnosticsLog(path_beside(model_path or "ppo_gail_model.pth"), SCHEDULE_COLUMNS if scheduled else ())
        sched = (tr.learning_rate(), tr.entropy_beta()) if scheduled else ()
    it, mean_rewards = 0, []
    while tr.episodes_lagged < num_episodes and (max_iterations is None or it < max_iterations):
        tr.train_iteration()
        if eval_log is not None:
            eval_log.add(tr.eval_tracker)
        if diag_log is not None:
            diag = tr.diagnostics()
            diag_log.add(it + 1, diag, sched)
            sched = (tr.learning_rate(), tr.entropy_beta()) if sched else ()      # the next update's
        if it % 10 == 0:
            ended = tr.buf["done"].sum().clamp(min=1.0)
            mean_rewards.append(float(tr.buf["rew"].sum() / ended))          # reward collected per episode ended in this rollout
            tr.losses()
            el, pl, acc = tr.disc_losses()
            rate = tr.successes_done / max(tr.episodes_done, 1)
            print(f"Episode {it} | Mean Reward: {mean_rewards[-1]:.2f} | Success Rate: {rate:.2%}")
            print(f"  episodes {tr.episodes_done} | radius {tr.radius:.1f} | D expert {el:.4f} policy {pl:.4f} accuracy {acc:.3f}"
                  + (f" | {progress_text(diag)}" if diag is not None else ""))
        it += 1
    if diag_log is not None:
        diag_log.close()
    if eval_log is not None:
        eval_log.close(tr.eval_tracker)
        curve = tr.eval_tracker.curve()
        if KEEP_BEST and model_path and curve and curve[-1]["state"][4] > 0:       # some evaluation became the best
            save_best_model(tr.eval_tracker, model_path)
    tr.losses()
    tr.disc_losses()
    for path, sd in ((model_path, tr.policy.state_dict()), (disc_path, tr.disc.state_dict())):
        if path:
            os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
            torch.save({k: v.cpu() for k, v in sd.items()}, path)
    if tr.reward_norm is not None and model_path:          # config.NORMALISE_REWARDS: the running state beside the policy
        from uavppo.reward_norm import save_state
        save_state(tr.reward_norm, model_path)
    if tr.obs_norm is not None and model_path:             # config.NORMALISE_OBS: the saved policy is the folded one; state and master beside it
        from uavppo.obs_norm import save_state as save_obs_state
        save_obs_state(tr.obs_norm, model_path)
    if tr.lr_control is not None and model_path:           # config.LR_SCHEDULE "adaptive": the rate the run ended at and the rule's counters
        from uavppo.lr_control import save_state as save_lr_state
        save_lr_state(tr.lr_control, model_path)
    print(f"training finished: {tr.episodes_done} episodes, {it} iterations; policy saved as {model_path}, discriminator as {disc_path}")
    return tr


def _main(argv):
    import argparse
    ap = argparse.ArgumentParser(description="PPO + GAIL (vectorised)")
    ap.add_argument("--episodes", type=int, default=2000)
    ap.add_argument("--num-envs", type=int, default=NUM_ENVS)
    ap.add_argument("--horizon", type=int, default=HORIZON)
    ap.add_argument("--expert", default="expert_data.npz")
    ap.add_argument("--policy", default=POLICY, choices=("mlp", "lstm"))
    ap.add_argument("--hidden", type=int, default=HIDDEN)
    ap.add_argument("--gail-coef", type=float, default=1.0)
    ap.add_argument("--env-coef", type=float, default=1.0)
    ap.add_argument("--max-iterations", type=int, default=None)
    ap.add_argument("--update-form", default="update_model", choices=("update_model", "inline_v10"))
    ap.add_argument("--minibatch-rows", type=int, default=None, help="shuffled row minibatches of this size (MLP policy)")
    ap.add_argument("--model-path", default="ppo_gail_model.pth")
    ap.add_argument("--disc-path", default="discriminator.pth")
    a = ap.parse_args(argv)
    train_ppo_gail(a.episodes, a.num_envs, a.horizon, a.expert, a.policy, a.hidden, a.gail_coef, a.env_coef,
                   max_iterations=a.max_iterations, model_path=a.model_path, disc_path=a.disc_path, update_form=a.update_form,
                   minibatch_rows=a.minibatch_rows)


if __name__ == "__main__":
    import sys
    os.environ["KMP_DUPLICATE_LIB_OK"] = "TRUE"
    _main(sys.argv[1:])
