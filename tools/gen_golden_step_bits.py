"""Record tests/golden/step_bits.json: SHA-256 digests of everything the policy-step kernels write, route by route.

The five kernels that take an env from "logits of this step" to "state of the next step" (rollout_lstm_kernel,
rollout_mlp_kernel, rollout_tail_kernel, greedy_tail_kernel, env_step_kernel) share their per-env arithmetic through the
core headers of csrc/.  Route-against-route tests cannot see a mistake all routes share, so tests/test_gpu_step_bits.py
compares every output buffer and the env state blob of each route with the digests recorded here -- by the build BEFORE a
change to that shared code, on the GPU:

    python tools/gen_golden_step_bits.py          # at the parent commit of the change

Inputs come from numpy's RandomState and the kernels' own counter RNG; nothing outside the repository is read.  A case's
seed is searched (0, 1, ..) until the run walks the branches the test wants walked -- FACTS below -- and is stored with the
digests; the file is not written unless every case finds one.
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "uav-wrf-les-ppo-lstm_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

DEV = "cuda:0"
PATH = os.path.join(ROOT, "tests", "golden", "step_bits.json")
RADIUS = 200.0          # of ~20 sources drawn in [50, 450]^2 a few lie this close to the start corner: those episodes end at once
N_ROLL, T_ROLL = 20, 24  # two workgroups of the fused kernels, the second with 12 dead lanes
N_TAIL = 18             # the tails' last wave is 2 envs short
INACTIVE = (1, 4, 7, 13, 17, 19)   # greedy: envs that come in with active = 0, in both workgroups
MAX_SEED = 64

# what a run must have walked, by kind of case (each a bool the case computes from its own outputs)
FACTS = {
    "rollout": ("auto_reset_before_last_step",),
    "greedy": ("ended_by_done", "active_to_the_end"),
    "greedy_rule": ("ended_by_done", "ended_by_hit", "active_to_the_end"),
    "env_step": ("auto_reset_before_last_step",),
}


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _uni(rs, shape, bound):
    return rs.uniform(-bound, bound, size=shape).astype(np.float32)


def _lstm_params(rs, H, D, head_gain=4.0):
    b = 1.0 / np.sqrt(H)
    parts = [_uni(rs, (4 * H, D), b), _uni(rs, (4 * H, H), b), _uni(rs, 4 * H, b), _uni(rs, 4 * H, b),
             _uni(rs, (6, H), head_gain * b), _uni(rs, 6, 0.5)]
    return _dev(np.concatenate([p.reshape(-1) for p in parts]))


def _mlp_params(rs, D):
    """W1[256][D] b1 g1 be1 W2[128][256] b2 g2 be2 Wh[6][128] bh (csrc/mlp.hip's flat layout)"""
    parts = [_uni(rs, (256, D), 1.0 / np.sqrt(D)), _uni(rs, 256, 0.1), 1.0 + _uni(rs, 256, 0.1), _uni(rs, 256, 0.1),
             _uni(rs, (128, 256), 1.0 / 16.0), _uni(rs, 128, 0.1), 1.0 + _uni(rs, 128, 0.1), _uni(rs, 128, 0.1),
             _uni(rs, (6, 128), 0.4), _uni(rs, 6, 0.5)]
    return _dev(np.concatenate([p.reshape(-1) for p in parts]))


def _env(N, variant, trend_k, seed, f64_bonus=False):
    from uavppo import ops
    state = torch.zeros(ops.env_state_bytes(N), dtype=torch.uint8, device=DEV)
    cfg = ops.make_env_cfg(variant, RADIUS, np.float64(0.6) if f64_bonus else 0.6, seed=1000 + seed, trend_k=trend_k)
    obs = torch.zeros(N, 6 + trend_k, device=DEV)
    ops.env_reset(state, N, cfg, obs)
    return state, cfg, obs


def _digests(**bufs):
    torch.cuda.synchronize()
    return {k: _sha(v) for k, v in bufs.items()}


# ------------------------------------------------------------------------------------------------ the fused training rollouts
def _rollout(seed, kind, hidden=0, trend_k=0, given=False, exact=False):
    """uav_rollout: kind 'lstm' (hidden 64 / 128) or 'mlp' (6 + trend_k inputs; exact = the f32-MFMA arithmetic).
    given: forced_act + noise instead of the counter RNG."""
    from uavppo import ops
    rs = np.random.RandomState(seed)
    N, T, D = N_ROLL, T_ROLL, 6 + trend_k
    state, cfg, cur = _env(N, "v2.1" if trend_k else "v2.0", trend_k, seed, f64_bonus=trend_k == 2)
    bufs = {"obs": torch.zeros(N, T, D, device=DEV), "act": torch.zeros(N, T, dtype=torch.int32, device=DEV),
            "flags": torch.zeros(N, T, dtype=torch.uint8, device=DEV)}
    for k in ("rew", "val", "logp", "done", "keep"):
        bufs[k] = torch.zeros(N, T, device=DEV)
    extra = {"last_val": torch.zeros(N, device=DEV), "info": torch.zeros(N, T, 10, device=DEV), "heads": torch.zeros(N, T, 6, device=DEV),
             "nan_count": torch.zeros(1, dtype=torch.int32, device=DEV)}
    forced = _dev(rs.randint(0, 5, size=(N, T)), torch.int32) if given else None
    noise = _dev(rs.randn(N, T, 2)) if given else None
    if kind == "lstm":
        params = _lstm_params(rs, hidden, D)
        h, c = _dev(_uni(rs, (N, hidden), 0.5)), _dev(_uni(rs, (N, hidden), 0.5))
        if given:                       # with the BPTT stash, so the stash / y stores and the TREND h_prev slot are recorded too
            extra["stash"], extra["y"] = torch.zeros(N, T, 6 * hidden, device=DEV), torch.zeros(N, T, hidden, device=DEV)
        ops.rollout_lstm(state, N, cfg, params, hidden, T, 3, cur, h, c, bufs, forced_act=forced, noise=noise, **extra)
        extra.update(h=h, c=c)
    else:
        params = _mlp_params(rs, D)
        bufs.pop("keep")
        with ops.lstm_arith("f32_mfma" if exact else "fp16x3"):
            ops.rollout_mlp(state, N, cfg, params, T, 3, cur, bufs, forced_act=forced, noise=noise, trend=trend_k != 0, **extra)
    d = _digests(state=state, cur_obs=cur, **bufs, **extra)
    done = bufs["done"].cpu().numpy()
    return d, {"auto_reset_before_last_step": bool(done[:, :T - 1].any())}


# ------------------------------------------------------------------------------------------------ the fused greedy episodes
def _greedy(seed, hidden, rule):
    """uav_greedy_episodes / _stop: 24 steps in two launches of 12, LSTM (hidden 64) or the MLP (hidden 0)."""
    from uavppo import ops
    rs = np.random.RandomState(seed)
    N, K = N_ROLL, T_ROLL // 2
    state, cfg, cur = _env(N, "v2.0", 0, seed)
    params = _lstm_params(rs, hidden, 6, head_gain=40.0) if hidden else _mlp_params(rs, 6)
    h = torch.zeros(N, hidden, device=DEV) if hidden else None
    c = torch.zeros(N, hidden, device=DEV) if hidden else None
    active = torch.ones(N, dtype=torch.uint8, device=DEV)
    active[list(INACTIVE)] = 0
    nan = torch.zeros(1, dtype=torch.int32, device=DEV)
    out, flags = {}, []
    if rule:
        # window 4; a std bound no 4 moves of 25 px exceed, so the concentration half decides: obs[2] > 0.06, a few % of cells
        R = ops.make_stop_rule(window=4, pos_std_max=1e3, conc_min=1200.0)
        win, cnt = torch.zeros(N, 4, 2, device=DEV), torch.zeros(N, dtype=torch.int32, device=DEV)
    for chunk in range(2):
        recs = {"act": torch.zeros(N, K, dtype=torch.int32, device=DEV), "obs": torch.zeros(N, K, 6, device=DEV),
                "pos": torch.zeros(N, K, 2, device=DEV), "flags": torch.zeros(N, K, dtype=torch.uint8, device=DEV)}
        if rule:
            rv = torch.zeros(N, K, device=DEV)
            ops.greedy_episodes_stop(state, N, cfg, params, hidden, K, cur, h, c, active, recs, R, win, cnt, noise=_dev(rs.randn(N, K, 2)),
                                     nan_count=nan, rule_val=rv)
            recs["rule_val"] = rv
        else:
            ops.greedy_episodes(state, N, cfg, params, hidden, K, cur, h, c, active, recs, nan_count=nan)
        torch.cuda.synchronize()
        for k, v in recs.items():
            out[f"{k}.{chunk}"] = _sha(v)
        flags.append(recs["flags"].cpu().numpy())
    last = {"state": state, "cur_obs": cur, "active": active, "nan_count": nan}
    if hidden:
        last.update(h=h, c=c)
    if rule:
        last.update(stop_win=win, stop_cnt=cnt)
    out.update(_digests(**last))
    fl = np.concatenate(flags, 1)
    facts = {"ended_by_done": bool((fl & 1).any()), "active_to_the_end": bool(active.any().item())}
    if rule:
        facts["ended_by_hit"] = bool((fl & 8).any())
    return out, facts


# ------------------------------------------------------------------------------------------------ the step-wise routes' tails
def _rollout_tail(seed, n_act, given):
    """uav_rollout_tail, steps t = 0, 1 of a T = 3 buffer; n_act 6 runs on the 8-feature observation."""
    from uavppo import ops
    rs = np.random.RandomState(seed)
    N, T, H, A1 = N_TAIL, 3, 64, n_act + 1
    trend_k = 2 if n_act == 6 else 0
    D = 6 + trend_k
    state, cfg, cur = _env(N, "v2.0", trend_k, seed)
    y = _dev(rs.randn(N, T, H).astype(np.float32))
    W, b = _dev(_uni(rs, (A1, H), 0.5)), _dev(_uni(rs, A1, 0.5))
    z = {"heads": torch.zeros(N, T, A1, device=DEV), "act_out": torch.zeros(N, dtype=torch.int32, device=DEV),
         "obs_seq": torch.zeros(N, T, D, device=DEV), "keep": torch.ones(N, device=DEV),
         "act": torch.zeros(N, T, dtype=torch.int32, device=DEV), "flags": torch.zeros(N, T, dtype=torch.uint8, device=DEV),
         "nan_count": torch.zeros(1, dtype=torch.int32, device=DEV)}
    for k in ("val", "logp", "keep_buf", "rew", "done"):
        z[k] = torch.zeros(N, T, device=DEV)
    for t in range(2):
        forced = _dev(rs.randint(-1, n_act + 1, size=N), torch.int32) if given else None     # with values the clamps catch
        noise = _dev(rs.randn(N, 2)) if given else None
        ops.rollout_tail(state, cfg, y, t, W, b, z["heads"], z["act_out"], cur, z["obs_seq"], z["keep"], z["act"], z["val"], z["logp"],
                         z["keep_buf"], z["rew"], z["done"], z["flags"], z["nan_count"], seed=77, iteration=5, index_offset=0,
                         forced_act=forced, noise=noise)
    d = _digests(state=state, cur_obs=cur, **z)
    return d, {"auto_reset_before_last_step": bool(z["done"].cpu().numpy()[:, 0].any())}


def _greedy_tail(seed, n_act, rule):
    """uav_greedy_tail, steps t = 0, 1 of a 2-column record; three envs come in inactive."""
    from uavppo import ops
    rs = np.random.RandomState(seed)
    N, K, H, A1 = N_TAIL, 2, 64, n_act + 1
    trend_k = 2 if n_act == 6 else 0
    D = 6 + trend_k
    state, cfg, cur = _env(N, "v2.0", trend_k, seed)
    W, b = _dev(_uni(rs, (A1, H), 0.5)), _dev(_uni(rs, A1, 0.5))
    active = torch.ones(N, dtype=torch.uint8, device=DEV)
    active[[2, 9, 17]] = 0
    recs = {"act": torch.zeros(N, K, dtype=torch.int32, device=DEV), "obs": torch.zeros(N, K, D, device=DEV),
            "pos": torch.zeros(N, K, 2, device=DEV), "flags": torch.zeros(N, K, dtype=torch.uint8, device=DEV)}
    last = {"nan_count": torch.zeros(1, dtype=torch.int32, device=DEV)}
    kw = {}
    if rule:                                              # window 2: full at the second step; obs[2] > 0.04 there is a hit
        kw = dict(rule=ops.make_stop_rule(window=2, pos_std_max=1e3, conc_min=800.0), stop_win=torch.zeros(N, 2, 2, device=DEV),
                  stop_cnt=torch.zeros(N, dtype=torch.int32, device=DEV), rule_val=torch.zeros(N, K, device=DEV))
        last.update(stop_win=kw["stop_win"], stop_cnt=kw["stop_cnt"], rule_val=kw["rule_val"])
    for t in range(2):
        y = _dev(rs.randn(N, H).astype(np.float32))
        noise = _dev(rs.randn(N, 2)) if t else None
        ops.greedy_tail(state, cfg, y, W, b, t, cur, active, recs, last["nan_count"], noise=noise, **kw)
    d = _digests(state=state, cur_obs=cur, active=active, **recs, **last)
    fl = recs["flags"].cpu().numpy()
    facts = {"ended_by_done": bool((fl & 1).any()), "active_to_the_end": bool(active.any().item())}
    if rule:
        facts["ended_by_hit"] = bool((fl & 8).any())
    return d, facts


def _env_step(seed, given):
    """uav_env_step, two steps; the actions include values outside 0 .. 4."""
    from uavppo import ops
    rs = np.random.RandomState(seed)
    N = N_TAIL
    state, cfg, obs = _env(N, "v2.0", 0, seed)
    out, dones = {}, []
    for t in range(2):
        z = {"obs": torch.zeros(N, 6, device=DEV), "rew": torch.zeros(N, device=DEV), "done": torch.zeros(N, device=DEV),
             "flags": torch.zeros(N, dtype=torch.uint8, device=DEV), "info": torch.zeros(N, 5, device=DEV),
             "term_obs": torch.zeros(N, 6, device=DEV), "rew64": torch.zeros(N, dtype=torch.float64, device=DEV)}
        act = _dev(rs.randint(-1, 7, size=N), torch.int32)
        ops.env_step(state, N, cfg, act, z["obs"], z["rew"], z["done"], z["flags"], noise=_dev(rs.randn(N, 2)) if given else None,
                     info=z["info"], term_obs=z["term_obs"], rew64=z["rew64"])
        torch.cuda.synchronize()
        out.update({f"{k}.{t}": _sha(v) for k, v in z.items()})
        dones.append(z["done"].cpu().numpy())
    out["state"] = _sha(state)
    return out, {"auto_reset_before_last_step": bool(dones[0].any())}


def cases():
    """name -> (kind of FACTS, callable(seed) -> (digests, facts))"""
    c = {}
    for H in (64, 128):
        for k in (0, 2):
            for given in (False, True):
                c[f"rollout_lstm-h{H}-k{k}-{'given' if given else 'philox'}"] = (
                    "rollout", lambda s, H=H, k=k, g=given: _rollout(s, "lstm", H, k, g))
    for k in (0, 2):
        for exact in (True, False):
            for given in (False, True):
                c[f"rollout_mlp-in{6 + k}-{'exact' if exact else 'h3'}-{'given' if given else 'philox'}"] = (
                    "rollout", lambda s, k=k, e=exact, g=given: _rollout(s, "mlp", 0, k, g, e))
    for name, H in (("lstm", 64), ("mlp", 0)):
        c[f"greedy-{name}"] = ("greedy", lambda s, H=H: _greedy(s, H, False))
        c[f"greedy_stop-{name}"] = ("greedy_rule", lambda s, H=H: _greedy(s, H, True))
    for A in (5, 6):
        c[f"rollout_tail-a{A}-philox"] = ("rollout", lambda s, A=A: _rollout_tail(s, A, False))
        c[f"rollout_tail-a{A}-given"] = ("rollout", lambda s, A=A: _rollout_tail(s, A, True))
        c[f"greedy_tail-a{A}"] = ("greedy", lambda s, A=A: _greedy_tail(s, A, False))
        c[f"greedy_tail-a{A}-rule"] = ("greedy_rule", lambda s, A=A: _greedy_tail(s, A, True))
    c["env_step-philox"] = ("env_step", lambda s: _env_step(s, False))
    c["env_step-given"] = ("env_step", lambda s: _env_step(s, True))
    return c


def run_case(name, seed):
    """(digests, facts) of one case; facts has exactly the keys FACTS asks of its kind."""
    from uavppo import ops
    kind, fn = cases()[name]
    with ops.lstm_arith("fp16x3"):                        # whatever mode the environment started the handle in
        digests, facts = fn(seed)
    assert sorted(facts) == sorted(FACTS[kind]), (name, facts)
    return digests, facts


def main():
    out = {}
    for name in cases():
        for seed in range(MAX_SEED):
            digests, facts = run_case(name, seed)
            if all(facts.values()):
                again, _ = run_case(name, seed)
                assert again == digests, f"{name}: two runs of seed {seed} differ"
                out[name] = {"seed": seed, "sha256": digests}
                print(f"{name}: seed {seed}, {len(digests)} buffers")
                break
        else:
            raise SystemExit(f"{name}: no seed below {MAX_SEED} gives {FACTS[cases()[name][0]]}; nothing written")
    with open(PATH, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{PATH}: {len(out)} cases, {os.path.getsize(PATH)} bytes")


if __name__ == "__main__":
    main()
