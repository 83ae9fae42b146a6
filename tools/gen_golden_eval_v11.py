"""Record tests/golden/eval_v11.npz and eval_v11_results.csv from the reference's own PPOV1.1/evaluate_model.py.

Runs only where the reference tree is present (oracle/_refload.REF_ROOT); the tests read the recorded files, never the tree.
The reference's ModelEvaluator.run_evaluation runs untouched (its 2000-step cap included) with random-initialised
PPOActorCritic policies of several torch seeds under fixed numpy seeds.  Recording is done from outside, by wrapping
methods of the instances: env.reset (source_pos), env.step (agent_pos, obs[2], done) and _check_stop_condition (its
decision, and np.std(last positions, axis=0).mean() -- the expression of evaluate_model.py:32 -- over the same list).
`gym` is replaced by oracle/_refload's empty stand-in; numpy, torch and pandas are the installed ones (versions recorded).

    python tools/gen_golden_eval_v11.py
"""
import io
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

import numpy as np  # noqa: E402
import pandas as pd  # noqa: E402
import torch  # noqa: E402

from oracle import _refload  # noqa: E402

# (torch seed of the policy, numpy seed of the env draws, episodes)
RUNS = ((0, 100, 3), (1, 101, 3), (2, 102, 3), (3, 103, 3), (4, 104, 3), (5, 105, 3), (6, 106, 2))


def main():
    _refload._install_third_party_stubs()
    ref = os.path.join(_refload.REF_ROOT, "PPOV1.1")
    sys.path.insert(0, ref)
    import evaluate_model as em
    import model as M
    W = 10
    pos, obs2, done, pos_std, stop, ep_len = [], [], [], [], [], []
    source, pol_seed, csv_parts, rows = [], [], [], []
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            for tseed, nseed, episodes in RUNS:
                class Ev(em.ModelEvaluator):
                    def _load_model(self, path):
                        torch.manual_seed(path)
                        m = M.PPOActorCritic(6, 5)
                        m.eval()
                        return m

                np.random.seed(nseed)
                ev = Ev(tseed, eval_episodes=episodes)
                assert ev.position_window == W
                env = ev.env
                env_reset, env_step, check = env.reset, env.step, ev._check_stop_condition

                def reset():
                    s = env_reset()
                    source.append(np.asarray(env.source_pos, np.float64).copy())
                    pol_seed.append(tseed)
                    ep_len.append(0)
                    return s

                def step(a):
                    out = env_step(a)
                    assert env.agent_pos.dtype == np.float32 and out[0].dtype == np.float32
                    pos.append(env.agent_pos.copy())
                    obs2.append(out[0][2])
                    done.append(bool(out[2]))
                    ep_len[-1] += 1
                    return out

                def check_stop(traj):
                    r = check(traj)
                    v = np.float32("nan")
                    if len(traj) >= ev.position_window:
                        v = np.std([t["pos"] for t in traj[-ev.position_window:]], axis=0).mean()
                        assert v.dtype == np.float32
                    assert type(traj[-1]["conc"]) is np.float32
                    pos_std.append(v)
                    stop.append(bool(r))
                    return r

                env.reset, env.step, ev._check_stop_condition = reset, step, check_stop
                out = io.StringIO()
                so, sys.stdout = sys.stdout, out
                try:
                    ev.run_evaluation()
                finally:
                    sys.stdout = so
                txt = open("evaluation_results.csv").read()
                csv_parts.append(txt)
                rows.append(pd.read_csv(io.StringIO(txt), float_precision="round_trip"))
        finally:
            os.chdir(cwd)
    df = pd.concat(rows, ignore_index=True)
    n = len(df)
    assert n == len(ep_len) == len(source) and sum(ep_len) == len(pos) == len(stop) == len(pos_std)
    assert (df["steps"].to_numpy() == np.asarray(ep_len)).all()
    # one CSV of all runs: the lines the reference wrote, its header once, the episodes numbered through
    gold = os.path.join(ROOT, "tests", "golden")
    lines = [ln.split(",", 1)[1] for part in csv_parts for ln in part.splitlines()[1:]]
    assert len(lines) == n
    with open(os.path.join(gold, "eval_v11_results.csv"), "w", newline="") as f:
        f.write(csv_parts[0].splitlines()[0] + "\n")
        for i, ln in enumerate(lines):
            f.write(f"{i + 1},{ln}\n")
    df["final_conc"] = df["final_conc"].astype(np.float32)
    np.savez_compressed(
        os.path.join(gold, "eval_v11.npz"),
        pos=np.asarray(pos, np.float32), obs2=np.asarray(obs2, np.float32), done=np.asarray(done, bool),
        pos_std=np.asarray(pos_std, np.float32), stop=np.asarray(stop, bool), ep_len=np.asarray(ep_len, np.int64),
        source_pos=np.asarray(source, np.float64), policy_seed=np.asarray(pol_seed, np.int64),
        steps=df["steps"].to_numpy(np.int64), deviation=df["deviation"].to_numpy(np.float64),
        success=df["success"].to_numpy(bool), final_conc=df["final_conc"].to_numpy(np.float32),
        radius=np.float64(ev.env.current_radius), window=np.int64(W), stability_threshold=np.float64(ev.stability_threshold),
        conc_threshold=np.float64(ev.conc_threshold), conc_peak=np.float64(em.CONC_PEAK), step_cap=np.int64(2000),
        numpy_version=np.array(np.__version__), torch_version=np.array(torch.__version__), pandas_version=np.array(pd.__version__))
    st = np.asarray(stop)
    ends = np.cumsum(ep_len) - 1
    print(f"{n} episodes, {len(pos)} steps; steps per episode {ep_len}; stopped by the rule {st[ends].tolist()}")


if __name__ == "__main__":
    main()
