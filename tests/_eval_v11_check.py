"""CPU restatement of PPOV1.1/evaluate_model.py's stop rule and episode bookkeeping (TEST INFRASTRUCTURE ONLY).

The rule on numpy f32 scalars, operation for operation what np.std(window, axis=0).mean() does for a [window][2] f32
array (sequential sums in time order, f32 division and sqrt), pinned bit for bit against the reference's recorded values
(tests/test_eval_v11_rule.py) and restated on the device in csrc/stop_rule_core.h; plus greedy oracle episodes over
OracleVecEnv with that rule, for the GPU tests.
"""
import numpy as np

F = np.float32
WINDOW, POS_STD_MAX, CONC_COEF, CONC_PEAK, CONC_MIN = 10, 2.0, 2.0, 100.0, 80.0


def pos_std(window):
    """np.std(window, axis=0).mean() of `window` f32 pairs (oldest first), restated."""
    w = np.asarray(window, F)
    n = F(len(w))
    s = np.zeros(2, F)
    for r in w:
        s = s + r
    mu = s / n
    q = np.zeros(2, F)
    for r in w:
        d = r - mu
        q = q + d * d
    sd = np.sqrt(q / n)
    return (sd[0] + sd[1]) / F(2)


def conc_of(obs2, coef=CONC_COEF, peak=CONC_PEAK):
    """trajectory[-1]['conc'] = info['concentration_reward'] * CONC_PEAK, f32 (evaluate_model.py:61)."""
    return (F(coef) * F(obs2)) * F(peak)


def conc_high(obs2, coef=CONC_COEF, peak=CONC_PEAK, conc_min=CONC_MIN):
    """(conc * CONC_PEAK > conc_threshold, conc * CONC_PEAK): the second scaling is the reference's (:35)."""
    v = conc_of(obs2, coef, peak) * F(peak)
    return bool(v > F(conc_min)), v


def rule(positions, obs2, window=WINDOW, pos_std_max=POS_STD_MAX, **kw):
    """(stop, pos_std or NaN) after the step that appended positions[-1] and returned obs[2] = obs2."""
    if len(positions) < window:
        return False, F("nan")
    v = pos_std(positions[-window:])
    return bool(v < F(pos_std_max)) and conc_high(obs2, **kw)[0], v


def episode_results(pos, obs2, done, source, radius, cap, window=WINDOW, pos_std_max=POS_STD_MAX):
    """evaluate_model.py:46-83 over recorded streams (pos [T][2] f32, obs2 [T] f32, done [T]) of ONE episode: walks them
    as the loop does and returns (steps, deviation, success, final_conc, stopped_by_rule, pos_std [steps], stop [steps])."""
    traj, vals, stops = [], [], []
    steps, over, fired = 0, False, False
    while not over and steps < cap:
        traj.append(np.asarray(pos[steps], F))
        over = bool(done[steps])
        fired, v = rule(traj, obs2[steps], window, pos_std_max)
        vals.append(v)
        stops.append(fired)
        if fired:
            over = True
        steps += 1
    d = traj[-1].astype(np.float64) - np.asarray(source, np.float64)
    deviation = float(np.sqrt(d[0] * d[0] + d[1] * d[1]))
    return steps, deviation, bool(deviation < radius), conc_of(obs2[steps - 1]), fired, np.asarray(vals, F), np.asarray(stops)


def oracle_episodes(policy_logits, bank, N, cap, noise, variant="v1.1", radius=50.0, window=WINDOW, pos_std_max=POS_STD_MAX):
    """One greedy episode per env of an OracleVecEnv over `bank` with the rule.  policy_logits() -> a fresh per-episode
    function obs f32 [6] -> f64 logits [5] (it may carry recurrent state).  noise f64 [cap][N][2].
    Returns a dict of per-env arrays (steps, stopped, success, reached, deviations, final_conc, pos [N][2]) and per-step
    [N][cap] arrays (rule_val f32, NaN where not stepped / window not full; flags u8 in the kernels' record format; pos_rec
    [N][cap][2] f32 agent_pos after each step; obs2_rec [N][cap] f32, the obs[2] each step returned),
    plus the margins met: gap (smallest top-2 logit gap), std_margin (min |pos_std - pos_std_max|), conc_margin (min
    |conc * CONC_PEAK - CONC_MIN| / CONC_PEAK^2 / CONC_COEF, i.e. in units of obs[2])."""
    from oracle.env_oracle import OracleVecEnv
    ora = OracleVecEnv(N, bank, variant, radius=radius)
    ora.reset()
    out = {k: [] for k in ("steps", "stopped", "success", "reached", "deviations", "final_conc", "pos")}
    rule_val = np.full((N, cap), np.nan, F)
    flags = np.full((N, cap), 4, np.uint8)
    pos_rec = np.zeros((N, cap, 2), F)
    obs2_rec = np.zeros((N, cap), F)
    gap, std_margin, conc_margin = np.inf, np.inf, np.inf
    for i, e in enumerate(ora.envs):
        logits = policy_logits()
        state, traj, t, over, fired, rc = e.obs(), [], 0, False, False, False
        while not over and t < cap:
            z = np.asarray(logits(state), np.float64)
            top = np.sort(z)[-2:]
            gap = min(gap, float(top[1] - top[0]))
            state, _, over, rc, _ = e.step(int(np.argmax(z)), noise[t, i])
            traj.append(np.asarray(e.pos, F))
            pos_rec[i, t] = traj[-1]
            obs2_rec[i, t] = state[2]
            fired, v = rule(traj, state[2], window, pos_std_max)
            rule_val[i, t] = v
            if len(traj) >= window:
                std_margin = min(std_margin, abs(float(v) - pos_std_max))
                conc_margin = min(conc_margin, abs(float(conc_high(state[2])[1]) - CONC_MIN) / (CONC_PEAK * CONC_PEAK * CONC_COEF))
            flags[i, t] = (1 if over else 0) | (2 if rc else 0) | (8 if fired else 0)
            over = over or fired
            t += 1
        d = traj[-1].astype(np.float64) - np.asarray(e.source, np.float64)
        dev = float(np.sqrt(d[0] * d[0] + d[1] * d[1]))
        for k, val in (("steps", t), ("stopped", fired), ("success", dev < radius), ("reached", rc), ("deviations", dev),
                       ("final_conc", conc_of(state[2])), ("pos", traj[-1])):
            out[k].append(val)
    out = {k: np.asarray(v) for k, v in out.items()}
    out.update(rule_val=rule_val, flags=flags, pos_rec=pos_rec, obs2_rec=obs2_rec, gap=gap, std_margin=std_margin, conc_margin=conc_margin)
    return out
