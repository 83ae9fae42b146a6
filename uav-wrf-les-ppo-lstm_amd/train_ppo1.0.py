# train_ppo1.0.py -- the PPOV1.1 trainer with the INLINE PPO update (one env, MLP policy) on the HIP kernels.
#
# Counterpart of the reference's PPOV1.1/train_ppo1.0.py:24-177.  Its update (:63-141, and with the same text the policy side
# of train_ppo_gail.py:71-148) is not `_update_model`: it differs in four places, all kept here in `_update_inline`:
#   * GAE with a real bootstrap: the last step of the buffer takes V(next_state) from the model and its own done; earlier
#     steps keep the done[t+1] mask (:75-84)                                   -> uav_gae mode UAV_GAE_INLINE_V10;
#   * returns = advantages + values from the RAW advantage (:86), and
#   * advantages = (A - mean) / (std + 1e-8) with no guard (:89)               -> uav_adv_normalise_inline;
#   * every epoch draws torch.randperm(L).split(BATCH_SIZE) and each chunk of sample rows is one optimiser step (:92-136)
#                                                                              -> uav_mlp_ppo_grad_rows.
# The buffer is NOT flushed when an episode ends (an update spans episodes), the loop writes no CSV, and every success appends
# the model's state_dict to the list saved at the end (:149-152, :173).
#
# The one deliberate difference: buffer.store's log-prob and the kernel's new log-prob keep the project's Categorical form
# (probabilities renormalised, clamped to [eps, 1 - eps], eps = 1.19e-7) where the reference takes the plain log(p[a]) (:56,
# :111).  The two differ only where the taken action's probability lies outside [1.19e-7, 1 - 1.19e-7], or by an ulp from the
# renormalisation.  TensorBoard output (the SummaryWriter scalars and histograms of :31, :156-162) is out of scope.
import importlib.util
import os

import numpy as np
import torch

from config import (BATCH_SIZE, CLIP_EPSILON, ENTROPY_BETA, EPOCHS, GAMMA, LAMBDA, LEARNING_RATE, PPO_DIAGNOSTICS, SEED, TARGET_KL,
                    WINDOW_SIZE)
from environment import MethaneEnv
from model import PPOActorCritic, PPOBuffer, PPOTrainer
from uavppo import ops

_spec = importlib.util.spec_from_file_location("train_ppo2_0", os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                                           "train_ppo2.0.py"))
_t20 = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_t20)
ClipAdam = _t20.ClipAdam


def _update_inline(buffer, next_value, model, optimizer, perms=None, diag_out=None):
    """train_ppo1.0.py:64-141 on the GPU: GAE bootstrapped from next_value = V(next_state), returns from the raw advantage,
    unguarded normalisation, then EPOCHS x (one permutation of the L rows, cut into chunks of BATCH_SIZE, one optimiser step per
    chunk).  perms (parity tests): index tensors [L], one per epoch, consumed in order instead of torch.randperm(L).  Returns the
    loss sums (policy, value, entropy, NaN count) and chunk length of every optimiser step.
    diag_out (a list; train_ppo passes one when config.PPO_DIAGNOSTICS or config.TARGET_KL is set): the loss kernel's update
    diagnostics are summed per epoch (uav_set_ppo_diag, attached for the epochs only), config.TARGET_KL drops the remaining
    epochs once an epoch's approximate KL exceeds it (uavppo.trainer.kl_stop: one host read per epoch), and the dict of
    uavppo.trainer.diagnostics_from_sums is appended to the list."""
    states, actions, rewards, values, log_probs, dones = buffer.get()
    core = model.core
    dev = core.device
    if (core.in_dim, core.h1, core.h2, core.n_act) != (6, 256, 128, 5):
        raise RuntimeError("_update_inline: row minibatches exist for the reference's 6-256-128 network only (uav_mlp_ppo_grad_rows)")
    L = len(rewards)
    d = lambda t: t.to(dev).contiguous()                        # noqa: E731
    rew, val, done = d(rewards)[None], d(values)[None], d(dones)[None]
    nv = torch.as_tensor(next_value, dtype=torch.float32).reshape(1).to(dev)
    adv = ops.gae(rew, val, done, GAMMA, LAMBDA, "inline_v10", last_val=nv)                    # :72-84
    adv_n, ret = ops.adv_normalise_inline(adv, val, ops.adv_stats(adv))                        # :86, :89
    x, act, lp = d(states), d(actions.to(torch.int32)), d(log_probs)
    loss_sums = torch.zeros(4, dtype=torch.float64, device=dev)
    steps = []
    diag = diag_ep = target = None
    if diag_out is not None:
        from uavppo.trainer import check_target_kl, diagnostics_from_sums, kl_stop
        target = check_target_kl(TARGET_KL)
        diag = torch.zeros(ops.PPO_DIAG_N, dtype=torch.float64, device=dev)
        diag_ep = torch.zeros(EPOCHS, ops.PPO_DIAG_N, dtype=torch.float64, device=dev)
        ops.set_ppo_diag(diag)
    epochs_run = 0
    try:
        for e in range(EPOCHS):                                                                # :92-94
            perm = torch.as_tensor(perms.pop(0)) if perms is not None else torch.randperm(L)
            if perm.numel() != L:
                raise ValueError(f"_update_inline: a permutation of {perm.numel()} rows for a buffer of {L}")
            for rows in perm.to(dev, torch.int32).split(BATCH_SIZE):
                grad = ops.mlp_ppo_grad_rows(core.flat, x, act, lp, adv_n.reshape(-1), ret.reshape(-1), val.reshape(-1),
                                             rows.contiguous(), 1.0 / rows.numel(), CLIP_EPSILON, ENTROPY_BETA, loss_sums, core.grad)
                if diag is not None:
                    diag_ep[e] += diag
                if isinstance(optimizer, ClipAdam):                                            # :133-136
                    optimizer.step_flat(core.flat, grad)
                else:                                                                          # a torch optimiser on model.parameters()
                    model.publish_grads()
                    torch.nn.utils.clip_grad_norm_(model.parameters(), 0.5)
                    optimizer.step()
                steps.append((loss_sums.clone(), rows.numel()))
            epochs_run = e + 1
            if target is not None and kl_stop(diag_ep[e].cpu().numpy(), target):
                break
    finally:
        if diag is not None:
            ops.set_ppo_diag(None)
    if diag_out is not None:
        diag_out.append(diagnostics_from_sums(diag_ep.cpu().numpy(), epochs_run=epochs_run))
    if any(s[3].item() > 0 for s, _ in steps):
        raise RuntimeError("NaN in probs")
    return steps


def train_ppo(episodes=2000, model_path="ppo_successful_models.pth", env=None, model=None, forced_actions=None, noise=None,
              max_steps_total=None):
    """forced_actions / noise (parity tests): recorded action stream and the env's step normals, consumed in order;
    max_steps_total stops after that many env steps (in the middle of an episode)."""
    env = env or MethaneEnv("v1.1")
    model = model or PPOActorCritic(6, 5)
    optimizer = ClipAdam(model.parameters(), lr=LEARNING_RATE)
    buffer = PPOBuffer()
    trainer = PPOTrainer(env, model, optimizer)
    gen = torch.Generator(device=model.core.device).manual_seed(SEED)
    # config.PPO_DIAGNOSTICS (or TARGET_KL): update_diagnostics.csv beside the saved models, one row per update
    diag_log, diag_out, diag_text = None, None, ""
    if PPO_DIAGNOSTICS or TARGET_KL is not None:
        from uavppo.update_log import UpdateDiagnosticsLog, path_beside, progress_text
        diag_log, diag_out = UpdateDiagnosticsLog(path_beside(model_path)), []
    success_count, episode_rewards, success_history, successful_models, t = 0, [], [], [], 0
    for episode in range(episodes):
        env.current_radius = trainer.current_radius                      # train_ppo1.0.py:45
        state = env.reset()
        done = False
        total_reward = 0.0
        while not done:
            st = torch.from_numpy(np.asarray(state, np.float32))[None]
            with torch.no_grad():
                probs, value = model(st)
            if forced_actions is not None:
                action = int(forced_actions[t])
            else:
                action = int(torch.multinomial(probs.to(model.core.device), 1, generator=gen).item())
            next_state, reward, done, _ = env.step(action, None if noise is None else noise[t])
            q = probs[0] / probs[0].sum()
            logp = float(torch.log(q.clamp(1.1920929e-07, 1 - 1.1920929e-07))[action])
            buffer.store(state, action, reward, value.item(), logp, done)
            state = next_state
            total_reward += reward
            t += 1
            if len(buffer.states) >= BATCH_SIZE:                         # :63-141
                with torch.no_grad():
                    next_value = model(torch.from_numpy(np.asarray(next_state, np.float32))[None])[1]
                _update_inline(buffer, next_value.reshape(-1), model, optimizer, diag_out=diag_out)
                buffer.clear()
                if diag_log is not None:
                    diag_log.add(len(diag_log.rows) + 1, diag_out[-1])
                    diag_text = " | " + progress_text(diag_out.pop())
            if max_steps_total is not None and t >= max_steps_total and not done:
                if diag_log is not None:
                    diag_log.close()
                return model, successful_models, trainer
        success = bool(env.trajectory[-1]["reached"])                   # :144-152
        trainer.update(success)
        success_history.append(success)
        if len(success_history) > WINDOW_SIZE:
            success_history.pop(0)
        if success:
            success_count += 1
            successful_models.append(model.state_dict())
        episode_rewards.append(total_reward)
        if episode % 10 == 0:                                            # :165-168
            print(f"Episode {episode} | Mean Reward: {np.mean(episode_rewards[-10:]):.2f} | "
                  f"Success Rate: {np.mean(success_history):.2%}" + diag_text)
    if diag_log is not None:
        diag_log.close()
    torch.save(successful_models, model_path)                            # :173
    print(f"training finished: {len(successful_models)} successful models saved to {model_path}")
    return model, successful_models, trainer


if __name__ == "__main__":
    train_ppo()
