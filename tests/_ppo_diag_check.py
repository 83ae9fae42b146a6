"""The eight update-diagnostic sums of include/uavppo.h (uav_set_ppo_diag) restated in f64 NumPy, and the inputs the tests of
tests/test_gpu_ppo_diag.py run the five loss-bearing entry points on.  Pure NumPy: tests/test_ppo_diag_host.py checks on the
CPU what the GPU tests assume about these inputs (no sample near a clip boundary, both sides of both clips populated).

logp is the Categorical(probs) log-probability of oracle/ppo_oracle.py:categorical_logp -- renormalise, clamp to
[eps, 1 - eps], log -- taken in f64 from the f32 inputs."""
import numpy as np

F32_EPS = float(np.finfo(np.float32).eps)
CLIP = 0.2
NAMES = ("kl_k1", "kl_k3", "clipped", "value_clipped", "verr2", "ret", "ret2", "count")
H1, H2, NA = 256, 128, 5
LN_EPS = 1e-5


def logp_f64(logits, act):
    z = np.asarray(logits, np.float64)
    p = np.exp(z - z.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    q = p / p.sum(-1, keepdims=True)
    q = np.clip(q, F32_EPS, 1.0 - F32_EPS)
    return np.log(q)[np.arange(len(q)), np.asarray(act, np.int64)]


def diag_sums(logits, value, act, logp_old, ret, val_old, clip=CLIP):
    """f64 [8] in the order of NAMES, from per-sample logits [n, A] and value [n] (any float dtype) and the f32 sample arrays."""
    lr = logp_f64(logits, act) - np.asarray(logp_old, np.float64)
    ratio = np.exp(lr)
    V, R, vo = (np.asarray(a, np.float64) for a in (value, ret, val_old))
    return np.array([(-lr).sum(), (np.expm1(lr) - lr).sum(), ((ratio < 1 - clip) | (ratio > 1 + clip)).sum(),
                     (np.abs(V - vo) > clip).sum(), ((R - V) ** 2).sum(), R.sum(), (R * R).sum(), float(len(lr))])


def clip_margin(logits, value, act, logp_old, val_old, clip=CLIP):
    """Smallest distance of a sample's ratio / |V - v_old| from a clip boundary: the counts are compared exactly, so no sample
    may sit where the kernel's f32 value and this f64 one could fall on different sides."""
    ratio = np.exp(logp_f64(logits, act) - np.asarray(logp_old, np.float64))
    dv = np.abs(np.asarray(value, np.float64) - np.asarray(val_old, np.float64))
    return float(min(np.abs(ratio - (1 - clip)).min(), np.abs(ratio - (1 + clip)).min(), np.abs(dv - clip).min()))


def sides(logits, value, act, logp_old, val_old, clip=CLIP):
    """(ratio below, ratio above, value below -clip, value above +clip) sample counts."""
    ratio = np.exp(logp_f64(logits, act) - np.asarray(logp_old, np.float64))
    dv = np.asarray(value, np.float64) - np.asarray(val_old, np.float64)
    return int((ratio < 1 - clip).sum()), int((ratio > 1 + clip).sum()), int((dv < -clip).sum()), int((dv > clip).sum())


def draw_samples(rng, logits, value):
    """act, logp_old, adv, ret, val_old (f32 / i32) for given per-sample heads: lr = logp - logp_old is N(0, 0.03) for nine
    samples in ten and +-U(0.15, 0.35) for the tenth (mean |lr| = 0.9 * 0.024 + 0.1 * 0.25 = 0.047: both sides of the ratio
    clip at exp(+-0.2) +- are populated without the bulk leaving the small-lr regime the k3 estimator is for); V - v_old likewise
    with N(0, 0.08) and +-U(0.25, 0.4).  From four samples on, samples 0 .. 3 are put on the four far sides by hand."""
    n = len(value)
    act = rng.randint(0, logits.shape[1], n).astype(np.int32)
    lp = logp_f64(logits, act)
    tail = rng.rand(n) < 0.1
    lr = np.where(tail, rng.choice([-1.0, 1.0], n) * rng.uniform(0.15, 0.35, n), 0.03 * rng.randn(n))
    tail = rng.rand(n) < 0.1
    dv = np.where(tail, rng.choice([-1.0, 1.0], n) * rng.uniform(0.25, 0.4, n), 0.08 * rng.randn(n))
    if n >= 4:
        lr[0], lr[1], dv[2], dv[3] = 0.3, -0.3, 0.3, -0.3
    V = np.asarray(value, np.float64)
    logp_old = (lp - lr).astype(np.float32)
    val_old = (V - dv).astype(np.float32)
    adv = rng.randn(n).astype(np.float32)
    ret = (V + 0.5 * rng.randn(n)).astype(np.float32)
    return act, logp_old, adv, ret, val_old


# ---------------------------------------------------------------------------------------------- the three kinds of heads
def heads_case(n, seed, A=5):
    """uav_ppo_loss: the heads are inputs."""
    rng = np.random.RandomState(seed)
    logits = rng.randn(n, A).astype(np.float32)
    value = rng.randn(n).astype(np.float32)
    act, lpo, adv, ret, vo = draw_samples(rng, logits, value)
    return dict(logits=logits, value=value, act=act, logp_old=lpo, adv=adv, ret=ret, val_old=vo,
                ref=diag_sums(logits, value, act, lpo, ret, vo), margin=clip_margin(logits, value, act, lpo, vo),
                sides=sides(logits, value, act, lpo, vo))


def from_y_case(n, H, seed):
    """uav_ppo_loss_from_y: heads = y W_head^T + b_head, here in f64."""
    rng = np.random.RandomState(seed)
    y = np.tanh(rng.randn(n, H)).astype(np.float32)
    w = (rng.randn(NA + 1, H) / np.sqrt(H)).astype(np.float32)
    b = (0.1 * rng.randn(NA + 1)).astype(np.float32)
    heads = y.astype(np.float64) @ w.astype(np.float64).T + b.astype(np.float64)
    logits, value = heads[:, :NA], heads[:, NA]
    act, lpo, adv, ret, vo = draw_samples(rng, logits, value)
    return dict(y=y, w_head=w, b_head=b, act=act, logp_old=lpo, adv=adv, ret=ret, val_old=vo,
                ref=diag_sums(logits, value, act, lpo, ret, vo), margin=clip_margin(logits, value, act, lpo, vo),
                sides=sides(logits, value, act, lpo, vo))


def mlp_params(in_dim, seed):
    """Flat f32 parameters in the layout of csrc/mlp.hip: W1[256][in] b1 g1 be1 W2[128][256] b2 g2 be2 Wh[6][128] bh[6], with
    non-trivial LayerNorm scales and biases."""
    rng = np.random.RandomState(seed)
    u = lambda shape, fan: rng.uniform(-1, 1, shape) / np.sqrt(fan)        # noqa: E731
    parts = [u((H1, in_dim), in_dim), 0.2 * rng.randn(H1), 1 + 0.3 * rng.randn(H1), 0.2 * rng.randn(H1),
             u((H2, H1), H1), 0.2 * rng.randn(H2), 1 + 0.3 * rng.randn(H2), 0.2 * rng.randn(H2),
             u((NA + 1, H2), H2), 0.2 * rng.randn(NA + 1)]
    return np.concatenate([p.reshape(-1) for p in parts]).astype(np.float32)


def mlp_heads_f64(flat, obs):
    """Linear -> LayerNorm -> ReLU, twice, then the six heads (PPOV2.0/model.py:17-53) in f64."""
    in_dim = obs.shape[1]
    f, o = np.asarray(flat, np.float64), 0

    def take(*shape):
        nonlocal o
        cnt = int(np.prod(shape))
        out = f[o:o + cnt].reshape(shape)
        o += cnt
        return out
    W1, b1, g1, be1 = take(H1, in_dim), take(H1), take(H1), take(H1)
    W2, b2, g2, be2 = take(H2, H1), take(H2), take(H2), take(H2)
    Wh, bh = take(NA + 1, H2), take(NA + 1)
    assert o == f.size

    def ln_relu(z, g, be):
        m, v = z.mean(-1, keepdims=True), z.var(-1, keepdims=True)
        return np.maximum((z - m) / np.sqrt(v + LN_EPS) * g + be, 0.0)
    a1 = ln_relu(np.asarray(obs, np.float64) @ W1.T + b1, g1, be1)
    a2 = ln_relu(a1 @ W2.T + b2, g2, be2)
    return a2 @ Wh.T + bh


def mlp_case(n, trend_k, seed, rows=None):
    """The fused MLP forms: n buffer rows; rows (i32 index, or None for all in order) are the launch's samples."""
    rng = np.random.RandomState(seed)
    D = 6 + trend_k
    flat = mlp_params(D, seed + 1)
    obs = rng.rand(n, D).astype(np.float32)
    obs[:, 6:] = 0.05 * rng.randn(n, trend_k)
    heads = mlp_heads_f64(flat, obs)
    logits, value = heads[:, :NA], heads[:, NA]
    act, lpo, adv, ret, vo = draw_samples(rng, logits, value)
    sel = np.arange(n) if rows is None else np.asarray(rows, np.int64)
    arg = (logits[sel], value[sel], act[sel], lpo[sel])
    return dict(params=flat, obs=obs, act=act, logp_old=lpo, adv=adv, ret=ret, val_old=vo, rows=rows,
                ref=diag_sums(*arg, ret[sel], vo[sel]), margin=clip_margin(*arg, vo[sel]), sides=sides(*arg, vo[sel]))


def rows_subset(n_total, n_rows, seed):
    """n_rows distinct buffer rows in shuffled order; rows 0 .. 3 (the samples put on the far sides by hand) are among them."""
    rng = np.random.RandomState(seed)
    rows = np.concatenate([np.arange(4), 4 + rng.permutation(n_total - 4)[:n_rows - 4]])
    return rng.permutation(rows).astype(np.int32)


# every case of the GPU tests: name -> builder (built once per session; the host test checks margins and sides of the same ones)
CASES = {
    "heads_n1": lambda: heads_case(1, 101),
    "heads_n1000": lambda: heads_case(1000, 102),            # 4 blocks of 256, the last one partial; 1020 of the 1024 partial rows unused
    "from_y_h64": lambda: from_y_case(300, 64, 103),         # one full 256-sample tile + a partial wave
    "from_y_h128": lambda: from_y_case(300, 128, 104),
    "mlp_k0_n1": lambda: mlp_case(1, 0, 105),                # the smallest n the entry takes: one partial 32-sample tile
    "mlp_k0_n33": lambda: mlp_case(33, 0, 106),              # a full tile + a tile of one sample (two workgroups)
    "mlp_k2_n1": lambda: mlp_case(1, 2, 107),
    "mlp_k2_n33": lambda: mlp_case(33, 2, 108),
    "mlp_rows": lambda: mlp_case(100, 0, 109, rows=rows_subset(100, 37, 9)),     # a permuted strict subset of the buffer rows
}
MARGIN = 1e-5


def compare(got, ref, n):
    """The GPU's eight sums against the restatement's.  Counts: exact.  The other five as MEANS, to the tolerance
    tests/test_gpu_update_kernels.py::test_ppo_loss_fwd_bwd applies to the loss sums (rtol 2e-5, atol 1e-6).  Returns the list
    of failures (empty = pass) after printing every figure."""
    bad = []
    for k, name in enumerate(NAMES):
        if name in ("clipped", "value_clipped", "count"):
            ok = got[k] == ref[k]
        else:
            ok = bool(np.isclose(got[k] / n, ref[k] / n, rtol=2e-5, atol=1e-6))
        print(f"  {name:14s} got {got[k]!r:26} ref {ref[k]!r:26} diff/n {(got[k] - ref[k]) / n:+.3e} {'ok' if ok else 'FAIL'}")
        if not ok:
            bad.append(name)
    return bad
