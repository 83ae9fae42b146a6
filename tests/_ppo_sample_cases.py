"""Case builders and f64 statements for the direct tests of the PPO loss, sampling, GAE and advantage kernels
(tests/test_gpu_loss_kernels.py runs them through uavppo.ops, tests/test_ppo_sample_cases_host.py checks the builders themselves on
the CPU).  Every input is generated in f32 and upcast for the f64 statement, so input rounding is no error.

The f64 statement of the loss is oracle.ppo_oracle.ppo_losses on f64 tensors (it clamps with f32's eps in any dtype) with torch
autograd for the gradients; the same function on f32 tensors on the CPU is the yardstick of tolerance (b):
    err_kernel <= 2 * err_torch_f32 + 2 f32 ulps of the compared scale            (check_b, as in tests/test_gpu_small_kernels.py)

A PPO sample next to one of the loss's branch points may take the other branch in f32, which moves its gradient by a whole term.
Nothing is left out of a comparison; `neutralise` changes such a sample's inputs instead so that either branch gives the same
answer, and at most CAP of a case's samples may be changed (the seeds below are chosen so; the host file asserts it)."""
import numpy as np
import torch

from oracle import ppo_oracle as po

F32, F64 = torch.float32, torch.float64
EPS = po.F32_EPS


def f32r(x):
    """a hyper-parameter as the f32 the C ABI receives, so that its rounding is no error"""
    return float(np.float32(x))


WIDTHS = (2, 3, 4, 5, 6, 8)                     # the action counts uav_ppo_loss / uav_policy_sample(_at) instantiate
LOSS_NS = (1, 255, 257, 5000)
FROM_Y_HS = (64, 128, 256)
FROM_Y_NS = (1, 15, 17, 63, 65, 255, 257, 1000)          # cut the 16-row MFMA tile, the 64-row wave, the 256-row block tile
FROM_Y_BIG = (262144 + 257, 64)                  # more than 1024 tiles of 256 rows: the block cap forces a second tile pass
CLIP, CLIP_DYADIC, BETA = f32r(0.2), 0.25, f32r(0.01)
NEAR = 1e-5                                      # a margin in f64 below which a branch decision counts as undecidable in f32
CAP = 1e-3                                       # the largest fraction of a case's samples `neutralise` may change


def ulp32(x):
    """the spacing of f32 at |x|"""
    return float(np.spacing(np.float32(abs(float(x)))))


def check_b(name, got, want, ref32, scale=None):
    """Tolerance (b).  got: the kernel's result, want: f64, ref32: f32 torch on the CPU; all CPU tensors of one shape.
    scale: what the 2-ulp floor is taken at (default: the largest |want|; a sum that cancels passes the sum of magnitudes)."""
    want = want.double()
    ek = float((got.double() - want).abs().max())
    et = float((ref32.double() - want).abs().max())
    floor = 2 * ulp32(float(want.abs().max()) if scale is None else scale)
    ratio = ek / et if et > 0 else float("inf") if ek > 0 else 0.0
    print(f"{name}: err_kernel {ek:.3e}  err_torch_f32 {et:.3e}  ratio {ratio:.2f}  floor {floor:.1e}")
    assert ek <= 2 * et + floor, (name, ek, et, floor)          # a NaN in `got` fails here too
    return ratio


# ----------------------------------------------------------------------------- the loss
def terms64(z64, v64, c, clip):
    """The quantities the loss branches on, in f64, from f64 logits [n, A] and values [n] and the case's other inputs."""
    q = torch.softmax(z64, -1)
    q = q / q.sum(-1, keepdim=True)
    qa = q.gather(1, c["act"].long()[:, None])[:, 0]
    logp = torch.log(qa.clamp(EPS, 1 - EPS))
    ratio = (logp - c["logp_old"].double()).exp()
    vo, ret = c["val_old"].double(), c["ret"].double()
    dv = v64 - vo
    vc = vo + dv.clamp(-clip, clip)
    return {"q": q, "qa": qa, "logp": logp, "ratio": ratio, "dv": dv, "e1": (v64 - ret) ** 2, "e2": (vc - ret) ** 2,
            "surrogate": torch.min(ratio * c["adv"].double(), ratio.clamp(1 - clip, 1 + clip) * c["adv"].double())}


def near_branch(z64, v64, c, clip):
    """(near a ratio clip edge, near a value branch point) as bool [n]: the samples whose branch f32 may decide otherwise"""
    t = terms64(z64, v64, c, clip)
    near_r = ((t["ratio"] - (1 - clip)).abs() < NEAR) | ((t["ratio"] - (1 + clip)).abs() < NEAR)
    outside = t["dv"].abs() > clip
    near_v = ((t["dv"].abs() - clip).abs() < NEAR) | (outside & ((t["e1"] - t["e2"]).abs() < NEAR))
    return near_r, near_v


def neutralise(z64, v64, c, clip):
    """adv = 0 next to a ratio clip edge (either branch then has the gradient 0), val_old = V next to |dv| = clip or to
    e1 = e2 outside the clip (dv = 0 then: an exact tie inside the clip whose two sides have one gradient) -> samples changed"""
    near_r, near_v = near_branch(z64, v64, c, clip)
    c["adv"][near_r] = 0.0
    c["val_old"][near_v] = v64[near_v].float()
    c["altered"] = int((near_r | near_v).sum())
    return c["altered"]


def _fill(c, z64, v64, g, clip):
    """the per-sample inputs of a random case around f64 logits / values: act, logp_old = the f64 log-probability + 0.25 randn,
    adv, ret = V + 0.5 randn, val_old = V + 0.3 randn; then `neutralise`"""
    n, A = z64.shape
    c["act"] = torch.randint(0, A, (n,), generator=g, dtype=torch.int32)
    logp = po.categorical_logp(torch.softmax(z64, -1), c["act"])
    c["logp_old"] = (logp + 0.25 * torch.randn(n, generator=g, dtype=F64)).float()
    c["adv"] = torch.randn(n, generator=g)
    c["ret"] = (v64 + 0.5 * torch.randn(n, generator=g, dtype=F64)).float()
    c["val_old"] = (v64 + 0.3 * torch.randn(n, generator=g, dtype=F64)).float()
    neutralise(z64, v64, c, clip)
    return c


# seeds of the random cases: n * 100 + A (+ H for from_y) unless that seed puts more than CAP of the samples next to a branch
# (0.1 % of 255 or 257 samples is none at all); the exceptions found on the CPU, checked by the host file
LOSS_SEED_EXCEPTIONS = {}
FROM_Y_SEED_EXCEPTIONS = {}


def loss_seed(n, A):
    return LOSS_SEED_EXCEPTIONS.get((n, A), n * 100 + A)


def from_y_seed(n, H):
    return FROM_Y_SEED_EXCEPTIONS.get((n, H), n * 1000 + H)


def loss_case(n, A, seed=None, clip=CLIP):
    """A random case of uav_ppo_loss: logits of scale 2, values of scale 1."""
    g = torch.Generator().manual_seed(loss_seed(n, A) if seed is None else seed)
    c = {"logits": 2.0 * torch.randn(n, A, generator=g), "value": torch.randn(n, generator=g)}
    return _fill(c, c["logits"].double(), c["value"].double(), g, clip)


def from_y_case(n, H, seed=None, clip=CLIP):
    """A random case of uav_ppo_loss_from_y: y [n, H] of scale 1, head weights [6, H] of scale 1 / sqrt(H) (heads of scale 1),
    biases of scale 0.1; the margins of `neutralise` are taken at the f64 heads."""
    g = torch.Generator().manual_seed(from_y_seed(n, H) if seed is None else seed)
    c = {"y": torch.randn(n, H, generator=g), "w": torch.randn(6, H, generator=g) / H ** 0.5, "b": 0.1 * torch.randn(6, generator=g)}
    heads = heads_of(c, F64)
    return _fill(c, heads[:, :5], heads[:, 5], g, clip)


def heads_of(c, dtype):
    return c["y"].to(dtype) @ c["w"].to(dtype).T + c["b"].to(dtype)


def heads_error_bound(c):
    """(a) How far a head formed in f32 may lie from y W^T + b [n, 6], read off ppo_loss_from_y_kernel (csrc/loss.hip), as
    colsum_chain does for uav_colsum.  The H products of a head are split over two accumulators; each takes H / 8 MFMA
    16x16x4 steps of four products, at most 8 roundings a step (four products, four additions; fewer where the unit fuses
    them), then the pair add and the bias: at most H + 2 roundings on the way into a head, each of at most 2^-24 of a partial
    sum, which is at most S = sum_u |y_u w_u| + |b|.  So |head - (y W^T + b)| <= (H + 2) 2^-24 S to first order in 2^-24.
    The bound holds for any order of the H additions (a sequential f32 dot product makes H + 1 roundings), so f32 torch's
    heads meet it too (asserted on the CPU)."""
    H = c["y"].shape[1]
    S = c["y"].double().abs() @ c["w"].double().abs().T + c["b"].double().abs()
    return (H + 2) * 2.0 ** -24 * S


def from_y_gradient_bound(c, clip=CLIP, beta=BETA):
    """(a) heads_error_bound propagated through the loss to first order: bound[i, j] = sum_k |d (n dheads[i, j]) / d heads[i, k]|
    * heads_error_bound[i, k], the derivatives by a second pass of f64 autograd (samples are independent, so the rows of the
    Jacobian are the gradients of the column sums of n dheads).  The second-order term is (H + 2) 2^-24 of the first."""
    heads = heads_of(c, F64).clone().requires_grad_(True)
    total = po.ppo_losses(torch.softmax(heads[:, :-1], -1), heads[:, -1], c["act"], c["logp_old"].double(), c["adv"].double(),
                          c["ret"].double(), c["val_old"].double(), clip, beta)[0]
    (g,) = torch.autograd.grad(total * heads.shape[0], heads, create_graph=True)
    dh = heads_error_bound(c)
    out = torch.zeros_like(dh)
    for j in range(g.shape[1]):
        (row,) = torch.autograd.grad(g[:, j].sum(), heads, retain_graph=True)
        out[:, j] = (row.abs() * dh).sum(1)
    return out


def loss_reference(c, dtype, clip=CLIP, beta=BETA):
    """ppo_losses + autograd in `dtype` -> {"sums": the three loss sums over n, "g": n * d total / d (logits | value) [n, A + 1],
    "dbias": the column sums of d total / d (logits | value)}.  A from_y case differentiates with respect to its heads."""
    if "y" in c:
        heads = heads_of(c, dtype)
        z, v = heads[:, :-1].clone().requires_grad_(True), heads[:, -1].clone().requires_grad_(True)
    else:
        z, v = c["logits"].to(dtype).clone().requires_grad_(True), c["value"].to(dtype).clone().requires_grad_(True)
    total, pl, vl, ent = po.ppo_losses(torch.softmax(z, -1), v, c["act"], c["logp_old"].to(dtype), c["adv"].to(dtype),
                                       c["ret"].to(dtype), c["val_old"].to(dtype), clip, beta)
    total.backward()
    n = z.shape[0]
    g = torch.cat([z.grad, v.grad[:, None]], 1)
    return {"sums": torch.stack([pl, vl, ent]).detach().double() * n, "g": g.double() * n, "dbias": g.sum(0)}


def sum_scales(c, clip=CLIP):
    """What the 2-ulp floor of the three loss sums is taken at: the sums of the terms' magnitudes (the surrogate's terms have
    either sign and cancel; the value loss's are non-negative already).  An entropy term p log(p + 1e-8) carries the rounding
    of p + 1e-8, an absolute 2^-24 p however small the logarithm is (at p = 1 f32 has log(1 + 1e-8) = 0), and the p of a
    sample add up to 1: the entropy sum's scale is at least n."""
    if "y" in c:
        heads = heads_of(c, F64)
        z64, v64 = heads[:, :-1], heads[:, -1]
    else:
        z64, v64 = c["logits"].double(), c["value"].double()
    t = terms64(z64, v64, c, clip)
    p = torch.softmax(z64, -1)
    return [float(t["surrogate"].abs().sum()), float(0.5 * torch.max(t["e1"], t["e2"]).sum()),
            max(float((p * torch.log(p + 1e-8)).abs().sum()), float(z64.shape[0]))]


def own_logp(c, dtype):
    """the log-probability of the case's own actions under its own logits, in `dtype`: as logp_old it makes every ratio exp(0)"""
    return po.categorical_logp(torch.softmax(c["logits"].to(dtype), -1), c["act"])


def ratio_one_case(n, A, seed):
    """Every first epoch's state: logp_old is the policy's own log-probability, every ratio exactly 1.  Logits of scale 3;
    the advantages are non-zero multiples of 1/8, so the surrogate sum -sum(adv) is exact in f64 in any order.  logp_old holds
    the f64 value rounded to f32; a caller replaces it by the log-probability of the arithmetic it runs."""
    g = torch.Generator().manual_seed(seed)
    c = {"logits": 3.0 * torch.randn(n, A, generator=g), "value": torch.randn(n, generator=g)}
    _fill(c, c["logits"].double(), c["value"].double(), g, CLIP)
    k = torch.randint(1, 33, (n,), generator=g).float() / 8
    c["adv"] = torch.where(torch.rand(n, generator=g) < 0.5, -k, k)
    c["logp_old"] = own_logp(c, F64).float()
    neutralise(c["logits"].double(), c["value"].double(), c, CLIP)          # the value side only: no ratio is near an edge
    assert (c["adv"] != 0).all()
    return c


# (val_old, V, ret, what the value gradient gV is): dyadic numbers with clip = 0.25, so every quantity below is exact in f32.
# d1 = 2 (V - R); inside the clip the clipped side has the same gradient d2 = d1, outside it d2 = 0.
VALUE_ROWS = [
    (1.0, 1.25, 0.5, "dv == +clip: in range, vc = V, e1 == e2, gV = 0.5 (d1 + d2) = 2 (V - R)"),
    (1.0, 0.75, 2.0, "dv == -clip: in range, vc = V, e1 == e2, gV = 2 (V - R)"),
    (0.0, 1.0, 0.0, "dv > clip, e1 > e2: gV = d1"),
    (0.0, 1.0, 1.5, "dv > clip, e1 < e2: gV = d2 = 0"),
    (0.0, 1.0, 0.625, "dv > clip, e1 == e2 (R midway between V and vc): gV = 0.5 (d1 + 0)"),
    (0.0, -1.0, 0.0, "dv < -clip, e1 > e2: gV = d1"),
    (0.0, -1.0, -1.5, "dv < -clip, e1 < e2: gV = 0"),
    (0.0, -1.0, -0.625, "dv < -clip, e1 == e2: gV = 0.5 d1"),
    (0.5, 0.5, -1.0, "dv == 0: gV = d1"),
    (1.0, 1.125, 3.0, "|dv| < clip: gV = d1"),
]
VALUE_GV = [1.5, -2.5, 2.0, 0.0, 0.375, -2.0, 0.0, -0.375, 3.0, -3.75]          # gV of each row, by hand


def value_clip_case(A, seed=11):
    """VALUE_ROWS with random logits of width A and clip = CLIP_DYADIC; the policy side is a plain random one."""
    n = len(VALUE_ROWS)
    g = torch.Generator().manual_seed(seed + A)
    c = {"logits": torch.randn(n, A, generator=g), "value": torch.tensor([r[1] for r in VALUE_ROWS])}
    _fill(c, c["logits"].double(), c["value"].double(), g, CLIP_DYADIC)
    c["val_old"] = torch.tensor([r[0] for r in VALUE_ROWS])
    c["ret"] = torch.tensor([r[2] for r in VALUE_ROWS])
    near_r, _ = near_branch(c["logits"].double(), c["value"].double(), c, CLIP_DYADIC)
    assert not near_r.any()
    return c


def value_clip_dvalue_f32(n):
    """dvalue of VALUE_ROWS as the kernel forms it in f32: (0.5 * inv_n) * gV, one rounding (gV itself is exact)"""
    inv_n = np.float32(1.0 / n)
    return np.float32(0.5) * inv_n * np.asarray(VALUE_GV, np.float32)


def clamp_case(A):
    """Logits [60, 0, ..., -60]: q of the first class is above 1 - eps, q of the last below eps, so Categorical's clamp is
    closed for an action at either end: no policy gradient, whatever the advantage; the entropy gradient remains.
    Rows: (first, adv 3), (last, adv 3), (first, adv -2), (last, adv -2); values well inside the clip."""
    z = torch.zeros(4, A)
    z[:, 0], z[:, -1] = 60.0, -60.0
    act = torch.tensor([0, A - 1, 0, A - 1], dtype=torch.int32)
    hi, lo = float(np.log(1 - EPS)), float(np.log(EPS))
    return {"logits": z, "value": torch.full((4,), 0.5), "act": act, "logp_old": torch.tensor([hi, lo, hi, lo]),
            "adv": torch.tensor([3.0, 3.0, -2.0, -2.0]), "ret": torch.ones(4), "val_old": torch.full((4,), 0.5)}


def overflow_case(A, sign, n=8, seed=5):
    """logp_old = -200: the f32 ratio exp(logp + 200) overflows to +inf (in f64 it is a finite 1e79 .. 1e87 that no f32 holds).
    sign: +1, -1 or 0 -- the sign of every advantage of the case."""
    g = torch.Generator().manual_seed(seed + A)
    c = {"logits": torch.randn(n, A, generator=g), "value": torch.randn(n, generator=g)}
    _fill(c, c["logits"].double(), c["value"].double(), g, CLIP)
    c["logp_old"] = torch.full((n,), -200.0)
    c["adv"] = sign * (0.5 + torch.rand(n, generator=g))
    _, near_v = near_branch(c["logits"].double(), c["value"].double(), c, CLIP)
    assert not near_v.any()
    return c


# ----------------------------------------------------------------------------- sampling
def sample_rows(n, A, seed):
    """logits [n, A] of scale 3 and uniforms [n] in [0, 1)"""
    g = torch.Generator().manual_seed(seed)
    return 3.0 * torch.randn(n, A, generator=g), torch.rand(n, generator=g)


def inverse_cdf_f32(probs, u):
    """sample_categorical's draw restated in f32 numpy from the kernel's own probs [n, A]: a sequential f32 psum, target =
    u * psum, a sequential f32 cdf, the first class with target < cdf, else A - 1 -- adds, one multiply and compares, all
    exactly rounded in numpy as on the device (the kernels are built without FMA contraction)."""
    probs, u = np.asarray(probs, np.float32), np.asarray(u, np.float32)
    n, A = probs.shape
    psum = np.zeros(n, np.float32)
    for k in range(A):
        psum = psum + probs[:, k]
    target = u * psum
    cdf = np.zeros(n, np.float32)
    act = np.full(n, A - 1, np.int64)
    found = np.zeros(n, bool)
    for k in range(A):
        cdf = cdf + probs[:, k]
        hit = ~found & (target < cdf)
        act[hit] = k
        found |= hit
    return act


def logp_argument_f32(probs, act):
    """the argument of the kernel's logf, from its own probs: q[a] = p[a] / psum (sequential f32 psum, one exactly rounded
    division), clamped to [eps, 1 - eps]"""
    probs = np.asarray(probs, np.float32)
    psum = np.zeros(probs.shape[0], np.float32)
    for k in range(probs.shape[1]):
        psum = psum + probs[:, k]
    qa = probs[np.arange(probs.shape[0]), np.asarray(act)] / psum
    return np.minimum(np.maximum(qa, np.float32(EPS)), np.float32(1) - np.float32(EPS))


U_LAST = float(np.nextafter(np.float32(1), np.float32(0)))      # the largest uniform the counter RNG's 24 bits give


def planted_sample_rows(A):
    """(logits [m, A], u [m], expected action or -1 where only the restatement decides):
    u = 0 with a first class of probability 0 must skip it; u just below 1; a last class of probability 0, where the
    fall-through (A - 1) and the last positive class (A - 2) differ; all logits equal."""
    ninf = float("-inf")
    rows, us, want = [], [], []

    def add(z, u, a):
        rows.append(z), us.append(u), want.append(a)
    base = [0.5 * k for k in range(A)]
    add([ninf] + base[1:], 0.0, 1)                              # target = 0 is not < cdf = 0
    add(base, 0.0, 0)
    add(base, U_LAST, A - 1)
    add([ninf] + base[1:], U_LAST, A - 1)
    if A > 2:
        add(base[:-1] + [ninf], U_LAST, -1)                     # A - 2 unless u * psum rounds up to psum: the restatement says
        add(base[:-1] + [ninf], 0.999, A - 2)
        add([ninf] + base[1:-1] + [ninf], 0.0, 1)
    for k in range(A):                                          # equal logits: class k owns [k / A, (k + 1) / A)
        add([1.25] * A, (k + 0.5) / A, k)
    add([1.25] * A, 0.0, 0)
    add([1.25] * A, U_LAST, A - 1)
    return torch.tensor(rows), torch.tensor(us), np.asarray(want)


# ----------------------------------------------------------------------------- GAE
GAE_TS = (1, 2, 63, 64, 65, 127, 129, 300)       # around the 64-step chunk of the wave scan: one, two, three and five chunks
GAE_NS = (1, 4, 5, 9)                            # around the 4 env rows of a block
GAE_P_DONE = (0.0, 0.1, 1.0)
GAE_COEFS = ((0.99, 0.95), (1.0, 1.0))           # with (1, 1) the scan's `a` products do not decay


def gae_case(n, T, p_done, seed):
    """rew of scale 2, val of scale 1, done with probability p_done; done on the last step for every other row and at t = 0
    of row 0 (for p_done < 1; with p_done = 1 every step is the last of its episode); last_val [n]"""
    rng = np.random.RandomState(seed)
    rew = (rng.randn(n, T) * 2).astype(np.float32)
    val = rng.randn(n, T).astype(np.float32)
    done = (rng.rand(n, T) < p_done).astype(np.float32)
    if p_done < 1:
        done[:, -1] = np.arange(n) % 2
        if T > 2:
            done[0, 0] = 1.0
    return rew, val, done, rng.randn(n).astype(np.float32)


def gae_f64(rew, val, done, last_val, gamma, lam, mode):
    """Each mode's recurrence as an f64 loop (rows at once); gamma and gamma * lam are the f32 values the kernel receives.
    mode "reference_exact": the mask and the value of step t come from step t + 1, the last step takes its own;
    "standard": mask done[t], bootstrap from last_val [n] (None: from 0)."""
    r, v, d = (np.asarray(x, np.float64) for x in (rew, val, done))
    g, gl = float(np.float32(gamma)), float(np.float32(gamma * lam))
    n, T = r.shape
    boot = np.zeros(n) if last_val is None else np.asarray(last_val, np.float64)
    adv, last = np.zeros((n, T)), np.zeros(n)
    for t in range(T - 1, -1, -1):
        if mode == "reference_exact":
            nnt = 1.0 - (d[:, t] if t == T - 1 else d[:, t + 1])
            nv = (v[:, t] if t == T - 1 else v[:, t + 1]) * nnt
        else:
            nnt = 1.0 - d[:, t]
            nv = (boot if t == T - 1 else v[:, t + 1]) * nnt
        last = (r[:, t] + g * nv - v[:, t]) + gl * nnt * last
        adv[:, t] = last
    return adv


# ----------------------------------------------------------------------------- advantage statistics and normalisation
# 1023 / 1025: around one block's 1024 elements a pass; 524288 + 1025 passes uav_adv_stats' 512-block cap (a second pass of
# its grid-stride loop), 2097152 + 513 the normalise kernels' 2048-block cap
ADV_NS = (1, 2, 1023, 1025, 524288 + 1025, 2097152 + 513)


def adv_case(n, seed=None):
    """adv of scale 3 around 1.5 (the sums grow with n), val of scale 1"""
    g = torch.Generator().manual_seed(n if seed is None else seed)
    return 3.0 * torch.randn(n, generator=g) + 1.5, torch.randn(n, generator=g)


def normalise_f64(adv, val, inline):
    """The formula in f64.  Whole-buffer form (train_ppo2.0.py:35-40): (A - mean) / (std + 1e-6), std = 1 if it is below 1e-6
    or NaN, returns = the normalised advantage + V.  Inline form (train_ppo1.0.py:86-89): returns = A + V from the raw
    advantage, (A - mean) / (std + 1e-8), no guard."""
    a, v = adv.double().reshape(-1), val.double().reshape(-1)
    std = a.std() if a.numel() > 1 else torch.tensor(float("nan"), dtype=F64)
    if inline:
        return (a - a.mean()) / (std + 1e-8), a + v
    if std < 1e-6 or torch.isnan(std):
        std = 1.0
    out = (a - a.mean()) / (std + 1e-6)
    return out, out + v


def normalise_f32(adv, val, inline):
    """the same operation in f32 torch on the CPU: the yardstick (the whole-buffer form is the oracle's `normalise`)"""
    if not inline:
        return po.normalise(adv, val)
    a, v = adv.reshape(-1), val.reshape(-1)
    std = a.std() if a.numel() > 1 else torch.tensor(float("nan"))
    return (a - a.mean()) / (std + 1e-8), a + v
