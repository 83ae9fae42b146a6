"""The inline PPO update of PPOV1.1/train_ppo1.0.py:63-141 restated in plain torch (CPU), in the dtype of the tensors it
is given: f32 meets the recording of the reference's own run (tests/golden/update_v10.npz, tools/gen_golden_train_v10.py),
f64 is what the GPU kernels are checked against.  Nothing here is drawn at random: the permutations are an input.

  gae_inline        :72-84   mask from done[t+1] and V[t+1]; the last step takes its own done and next_value
  normalise_inline  :86, :89 returns from the raw advantage; (A - mean) / (std + 1e-8), unbiased std, no guard
  losses            :110-130 clipped policy loss, entropy bonus, clipped value loss; total = policy - beta * entropy + value
  ClipAdam          :133-136 clip_grad_norm_(0.5) + torch.optim.Adam's arithmetic
  update            :92-141  EPOCHS x chunks of BATCH_SIZE rows of a permutation, one optimiser step per chunk

The log-prob of the taken action is the project's Categorical form (renormalise, clamp to [eps, 1 - eps], eps = 2^-23);
with probabilities inside that range it is the reference's log(p[a]) up to the renormalisation's rounding.
"""
import math

import torch
import torch.nn.functional as F

F32_EPS = 2.0 ** -23
KEYS = ("feature.0.weight", "feature.0.bias", "feature.1.weight", "feature.1.bias", "feature.3.weight", "feature.3.bias",
        "feature.4.weight", "feature.4.bias", "actor.weight", "actor.bias", "critic.weight", "critic.bias")


def forward(p, x):
    """probs [B, A], value [B] of the reference's PPOActorCritic (model.py:42-53) from a dict with its state_dict keys."""
    h = x
    for lin, ln in (("feature.0", "feature.1"), ("feature.3", "feature.4")):
        h = F.linear(h, p[lin + ".weight"], p[lin + ".bias"])
        h = F.relu(F.layer_norm(h, h.shape[-1:], p[ln + ".weight"], p[ln + ".bias"], 1e-5))
    probs = torch.softmax(F.linear(h, p["actor.weight"], p["actor.bias"]), -1)
    return probs, F.linear(h, p["critic.weight"], p["critic.bias"])[:, 0]


def gae_inline(rew, val, done, next_value, gamma=0.99, lam=0.95):
    """rew / val / done [n, T] (or [T]), next_value [n] (or a scalar) -> advantages of the same shape; the reference's
    operation order, python-float coefficients against tensors of the buffers' dtype."""
    one_d = rew.dim() == 1
    rew, val, done = (t.reshape(1, -1) if one_d else t for t in (rew, val, done))
    nv_last = torch.as_tensor(next_value, dtype=rew.dtype).reshape(-1)
    T = rew.shape[1]
    adv = torch.zeros_like(rew)
    gae = torch.zeros_like(rew[:, 0])
    for t in reversed(range(T)):
        if t == T - 1:
            nnt, nv = 1.0 - done[:, t], nv_last
        else:
            nnt, nv = 1.0 - done[:, t + 1], val[:, t + 1]
        delta = rew[:, t] + gamma * nv * nnt - val[:, t]
        gae = delta + gamma * lam * nnt * gae
        adv[:, t] = gae
    return adv[0] if one_d else adv


def normalise_inline(adv, val):
    """(normalised advantage, returns); one element gives NaN, as torch's unbiased std of one element does."""
    a = adv.reshape(-1)
    return ((a - a.mean()) / (a.std() + 1e-8)).reshape(adv.shape), adv + val


def losses(probs, value, act, logp_old, adv, ret, val_old, clip=0.2, beta=0.01):
    """(total, policy loss without the entropy term, value loss, entropy), all means over the batch."""
    q = (probs / probs.sum(-1, keepdim=True)).clamp(F32_EPS, 1 - F32_EPS)
    logp = torch.log(q).gather(1, act.long()[:, None])[:, 0]
    ratio = (logp - logp_old).exp()
    pl = -torch.min(ratio * adv, ratio.clamp(1 - clip, 1 + clip) * adv).mean()
    ent = -(probs * torch.log(probs + 1e-8)).sum(1).mean()
    vclip = val_old + (value - val_old).clamp(-clip, clip)
    vl = 0.5 * torch.max((value - ret).pow(2), (vclip - ret).pow(2)).mean()
    return pl - beta * ent + vl, pl, vl, ent


def grad_of(p, x, act, logp_old, adv, ret, val_old, clip=0.2, beta=0.01):
    """Autograd gradient of the total loss at p (not modified) -> (dict of gradients, (total, pl, vl, ent) as floats)."""
    leaf = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    probs, value = forward(leaf, x)
    out = losses(probs, value, act, logp_old, adv, ret, val_old, clip, beta)
    out[0].backward()
    return {k: leaf[k].grad for k in p}, tuple(float(t.detach()) for t in out)


class ClipAdam:
    """clip_grad_norm_(max_norm) then torch.optim.Adam (betas 0.9 / 0.999, eps 1e-8, no weight decay) over a dict."""

    def __init__(self, p, lr=3e-5, max_norm=0.5, b1=0.9, b2=0.999, eps=1e-8):
        self.lr, self.max_norm, self.b1, self.b2, self.eps, self.t = lr, max_norm, b1, b2, eps, 0
        self.m = {k: torch.zeros_like(v) for k, v in p.items()}
        self.v = {k: torch.zeros_like(v) for k, v in p.items()}

    def step(self, p, g):
        """p is updated in place; returns the gradient norm before clipping."""
        norm = torch.sqrt(sum((x * x).sum() for x in g.values()))
        coef = torch.clamp(self.max_norm / (norm + 1e-6), max=1.0)
        self.t += 1
        bc1, bc2 = 1 - self.b1 ** self.t, 1 - self.b2 ** self.t
        for k in p:
            gk = g[k] * coef
            self.m[k] = self.m[k] + (gk - self.m[k]) * (1 - self.b1)
            self.v[k] = self.v[k] * self.b2 + gk * gk * (1 - self.b2)
            denom = self.v[k].sqrt() / math.sqrt(bc2) + self.eps
            p[k] -= (self.lr / bc1) * (self.m[k] / denom)
        return float(norm)


def update(p, opt, states, actions, rewards, values, log_probs, dones, next_value, perms, batch_size=256, gamma=0.99, lam=0.95,
           clip=0.2, beta=0.01):
    """One inline update of the 1-d buffers: p (dict, updated in place) through len(perms) epochs.  Returns
    (advantages normalised, returns, [per optimiser step: dict(loss=(total, pl, vl, ent), gnorm, n, grad, params)])."""
    adv = gae_inline(rewards, values, dones, next_value, gamma, lam)
    adv_n, ret = normalise_inline(adv, values)
    steps = []
    for perm in perms:
        for idx in torch.as_tensor(perm).long().split(batch_size):
            at = {k: v.clone() for k, v in p.items()}
            g, ls = grad_of(p, states[idx], actions[idx], log_probs[idx], adv_n[idx], ret[idx], values[idx], clip, beta)
            steps.append(dict(loss=ls, n=len(idx), grad={k: v.clone() for k, v in g.items()}, params=at, gnorm=opt.step(p, g)))
    return adv_n, ret, steps
