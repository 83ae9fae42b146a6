"""Record tests/golden/update_v10.npz from the reference's own PPOV1.1/train_ppo1.0.py.

Runs only where the reference tree is present (oracle/_refload.REF_ROOT); the tests read the recorded file, never the tree.
The reference's train_ppo() runs untouched under fixed numpy and torch seeds, with `gym` replaced by oracle/_refload's empty
stand-in and torch.utils.tensorboard by a SummaryWriter that drops what it is given.  Recording is done from outside:

  PPOBuffer.get                   its six tensors, once per update;
  PPOActorCritic.forward          next_value = the value of the one forward pass made under no_grad per update (:67-70),
                                  and the smallest / largest probability of any forward pass;
  torch.randperm                  every permutation drawn (one per epoch);
  Tensor.backward                 the total loss of every optimiser step;
  clip_grad_norm_                 the gradient norm before clipping;
  Adam.step                       the model's state_dict before the first update and after each update; the run is stopped
                                  by raising a private exception from it after the 15th call (3 updates x 5 epochs: with
                                  BATCH_SIZE = 256 rows in the buffer a permutation splits into one chunk).

The generator asserts that every probability of the recording lies in [1e-4, 1 - 1e-4] (a freshly initialised actor, gain
0.01, gives about 0.2 each): there the project's clamp of the log-prob to [1.19e-7, 1 - 1.19e-7] is inert, so the recorded
update is the one the project's kernels compute.

    python tools/gen_golden_train_v10.py [numpy/torch seed]
"""
import importlib.util
import io
import os
import sys
import tempfile
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import _refload  # noqa: E402

UPDATES, STEPS = 3, 15
SEED = 277        # (the first seed of 0 .. 329 whose recording ends a buffer on a done: the first buffer, which also has one inside)


class _Stop(Exception):
    pass


def record(seed):
    """One run of the reference's train_ppo() under `seed`, stopped after the 15th optimiser step -> the arrays of the .npz."""
    _refload._install_third_party_stubs()
    tb = types.ModuleType("torch.utils.tensorboard")

    class SummaryWriter:
        def __init__(self, *a, **k):
            pass

        def add_scalar(self, *a, **k):
            pass

        add_histogram = add_scalar

        def close(self):
            pass

    tb.SummaryWriter = SummaryWriter
    sys.modules["torch.utils.tensorboard"] = tb
    ref = os.path.join(_refload.REF_ROOT, "PPOV1.1")
    sys.path.insert(0, ref)
    for m in ("config", "environment", "model"):
        sys.modules.pop(m, None)
    import config as C
    import model as M
    spec = importlib.util.spec_from_file_location("train_ref_v10", os.path.join(ref, "train_ppo1.0.py"))
    train = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(train)

    rec = dict(buffers=[], next_value=[], perms=[], loss=[], gnorm=[], sd=[], pmin=1.0, pmax=0.0, model=None)

    buf_get, fwd = M.PPOBuffer.get, M.PPOActorCritic.forward

    def get(self):
        out = buf_get(self)
        rec["buffers"].append([t.clone() for t in out])
        return out

    def forward(self, x):
        rec["model"] = self
        probs, value = fwd(self, x)
        rec["pmin"], rec["pmax"] = min(rec["pmin"], float(probs.detach().min())), max(rec["pmax"], float(probs.detach().max()))
        if not torch.is_grad_enabled():
            rec["next_value"].append(value.detach().reshape(-1).clone())
        return probs, value

    randperm, backward, clip = torch.randperm, torch.Tensor.backward, torch.nn.utils.clip_grad_norm_

    def rp(*a, **k):
        p = randperm(*a, **k)
        rec["perms"].append(p.clone())
        return p

    def bw(self, *a, **k):
        rec["loss"].append(float(self.detach()))
        return backward(self, *a, **k)

    def cg(params, max_norm, *a, **k):
        assert max_norm == 0.5
        n = clip(params, max_norm, *a, **k)
        rec["gnorm"].append(float(n))
        return n

    def snapshot():
        rec["sd"].append({k: v.detach().clone() for k, v in rec["model"].state_dict().items()})

    class RecAdam(torch.optim.Adam):
        calls = 0

        def step(self, *a, **k):
            if RecAdam.calls == 0:
                snapshot()
            out = super().step(*a, **k)
            RecAdam.calls += 1
            if RecAdam.calls % C.EPOCHS == 0:
                snapshot()
            if RecAdam.calls == STEPS:
                raise _Stop()
            return out

    M.PPOBuffer.get, M.PPOActorCritic.forward = get, forward
    train.optim = types.SimpleNamespace(Adam=RecAdam)
    torch.randperm, torch.Tensor.backward, torch.nn.utils.clip_grad_norm_ = rp, bw, cg
    np.random.seed(seed)
    torch.manual_seed(seed)
    cwd, so = os.getcwd(), sys.stdout
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        sys.stdout = io.StringIO()
        try:
            train.train_ppo()
            raise AssertionError("the reference's loop ended by itself")
        except _Stop:
            pass
        finally:
            sys.stdout = so
            os.chdir(cwd)
            torch.randperm, torch.Tensor.backward, torch.nn.utils.clip_grad_norm_ = randperm, backward, clip
            M.PPOBuffer.get, M.PPOActorCritic.forward = buf_get, fwd

    assert len(rec["buffers"]) == len(rec["next_value"]) == UPDATES and len(rec["sd"]) == UPDATES + 1
    assert len(rec["perms"]) == len(rec["loss"]) == len(rec["gnorm"]) == STEPS
    assert all(len(p) == C.BATCH_SIZE for p in rec["perms"]), "one chunk per permutation"
    assert 1e-4 <= rec["pmin"] and rec["pmax"] <= 1 - 1e-4, (rec["pmin"], rec["pmax"])
    for b in rec["buffers"]:
        p = torch.exp(b[4])
        assert float(p.min()) >= 1e-4 and float(p.max()) <= 1 - 1e-4
    names = ("states", "actions", "rewards", "values", "log_probs", "dones")
    out = {n: np.stack([b[i].numpy() for b in rec["buffers"]]) for i, n in enumerate(names)}
    out["next_value"] = np.stack([v.numpy() for v in rec["next_value"]]).reshape(UPDATES).astype(np.float32)
    out["perms"] = np.stack([p.numpy() for p in rec["perms"]]).astype(np.int64)
    out["loss"] = np.asarray(rec["loss"], np.float64)
    out["gnorm"] = np.asarray(rec["gnorm"], np.float64)
    for k in rec["sd"][0]:
        out["sd." + k] = np.stack([sd[k].numpy() for sd in rec["sd"]])
    hp = dict(gamma=C.GAMMA, lam=C.LAMBDA, clip=C.CLIP_EPSILON, ent_beta=C.ENTROPY_BETA, lr=C.LEARNING_RATE)
    for k, v in hp.items():
        out[k] = np.float64(v)
    out["batch_size"], out["epochs"], out["seed"] = np.int64(C.BATCH_SIZE), np.int64(C.EPOCHS), np.int64(seed)
    out["versions"] = np.array(f"numpy {np.__version__} torch {torch.__version__}")
    out["prob_range"] = np.asarray([rec["pmin"], rec["pmax"]], np.float64)
    return out


def main(seed=SEED):
    out = record(seed)
    # the recording must walk both branches of the last step's mask (train_ppo1.0.py:76-78): a buffer that ends on a done,
    # where V(next_state) must not enter, and one that does not
    assert out["dones"][:, -1].any() and not out["dones"][:, -1].all(), out["dones"][:, -1]
    path = os.path.join(ROOT, "tests", "golden", "update_v10.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes; dones per buffer {out['dones'].sum(1).tolist()}, last-step done "
          f"{out['dones'][:, -1].tolist()}; probabilities in {out['prob_range'].tolist()}; losses {out['loss'][:3].tolist()}")


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else SEED)
