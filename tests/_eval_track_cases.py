"""Synthetic greedy records and evaluation rows shared by tests/test_eval_track_host.py and tests/test_gpu_eval_track.py."""
import numpy as np

NAN = float("nan")
KINDS = ("end at record 0", "end at record k - 1", "nowhere", "bit3 alone", "bit3 with bit0", "bit3 before bit0",
         "bit2 records after an end", "comes in ended")


def records(n, k, D):
    """flags u8 [n, k], obs f32 [n, k, D], pos f32 [n, k, 2] that tell every (env, step) apart, env e of kind KINDS[e % 8] with its
    event at record p = (e // 8) % k; the obs / pos of every bit2 (not stepped) record are NaN.  Also the start state (ep_steps,
    ep_state, ep_pos): envs of the last kind come in ended and hold sentinel values that nothing may touch."""
    e, i = np.arange(n)[:, None], np.arange(k)[None, :]
    obs = np.zeros((n, k, D), np.float32)
    for j in range(D):
        obs[:, :, j] = ((8 * e + 2 * i + j + 1) / 4096.0).astype(np.float32)
    pos = np.stack([1000.0 + 8 * e + 2 * i, 1000.5 + 8 * e + 2 * i], 2).astype(np.float32)
    flags = np.zeros((n, k), np.uint8)
    kind = np.arange(n) % 8
    p = (np.arange(n) // 8) % k
    for env in range(n):
        q, kd = int(p[env]), int(kind[env])
        if kd == 0:
            flags[env, 0] = 1 | 2                       # done and reached
            flags[env, 1:] = 4
        elif kd == 1:
            flags[env, k - 1] = 1
        elif kd == 3:
            flags[env, q] = 8
            flags[env, q + 1:] = 4
        elif kd == 4:
            flags[env, q] = 9
            flags[env, q + 1:] = 4
        elif kd == 5:                                   # the rule's record first, a done record behind it: the first one counts
            flags[env, q] = 8
            if q + 1 < k:
                flags[env, k - 1] = 1
        elif kd == 6:
            flags[env, q] = 1
            flags[env, q + 1:] = 4
        elif kd == 7:                                   # ended before this chunk: whatever the records say
            flags[env, q] = 1
    skipped = (flags & 4) != 0
    obs[skipped] = NAN
    pos[skipped] = NAN
    ep_steps, ep_state, ep_pos = np.zeros(n, np.int32), np.zeros(n, np.uint8), np.zeros((n, 2), np.float64)
    ended = kind == 7
    ep_steps[ended] = 7
    ep_state[ended] = np.where(np.arange(n)[ended] % 16 == 7, 1, 3).astype(np.uint8)
    ep_pos[ended] = (np.arange(2 * int(ended.sum()), dtype=np.float64) - 99.0).reshape(-1, 2)
    return flags, obs, pos, (ep_steps, ep_state, ep_pos)


def sources(n):
    """f64 [n, 2] near the records' positions: some within 40 px of where an env ends, some not."""
    e = np.arange(n, dtype=np.float64)
    return np.stack([1000.0 + 8 * e + (e % 5) * 17.0, 1000.0 + 8 * e - (e % 3) * 11.0], 1)


def _row(episodes, successes, steps, nan=0.0, dev=10.0):
    return np.array([episodes, successes, steps, dev * episodes, dev * dev * episodes, dev * successes, 1.0, nan], np.float64)


# (iteration, sums row, took) in the order they are played: what uav_keep_best / better_rule must decide
RULE_TABLE = [
    (1, np.array([64.0, 3.0, 900.0, NAN, NAN, 12.0, 0.0, 0.0]), 0, "a NaN row"),
    (2, _row(64.0, 9.0, 500.0, nan=2.0), 0, "a row with sums[7] > 0"),
    (3, _row(0.0, 0.0, 0.0), 0, "a zero-episode row"),
    (4, _row(64.0, 5.0, 100.0), 1, "the first valid row"),
    (5, _row(64.0, 6.0, 200.0), 1, "strictly more successes"),
    (6, _row(64.0, 6.0, 150.0), 1, "a tie broken by steps"),
    (7, _row(64.0, 6.0, 150.0), 0, "a full tie keeps the earlier row"),
    (8, _row(64.0, 5.0, 10.0), 0, "fewer successes"),
    (9, np.array([64.0, 7.0, NAN, 1.0, 1.0, 1.0, 0.0, 0.0]), 0, "a NaN row after a best"),
]
RULE_FINAL_STATE = np.array([6.0, 150.0, 6.0, 9.0, 3.0, 4.0, 0.0])
