"""The h = 256 LSTM backward (fp16-split step kernels, gate gradients stored once as fp16 pieces with one power-of-two scale per
(env, step): lstm_forms.h DgPack, csrc/wgrad_pc.hip) against an f64 LSTM -- across the dispatch branches of the weight-gradient
pass, over 40 decades of gradient magnitude, with (env, step) rows whose gate gradients are exactly zero or NaN, and with a
stash whose h_prev slot the forward pass left unwritten.  -m gpu."""
import pytest
import torch

from oracle import ppo_oracle as po

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, A = 256, 6
GRADS = ("dx", "dw_ih", "dw_hh", "db", "dh0", "dc0", "dw_head")


@pytest.fixture(scope="module")
def ops():
    from uavppo import ops as o
    yield o
    o.set_lstm_arith("fp16x3")
    o.set_debug_flags()


def _problem(N, T, I, seed, fused, scale=1.0, restarts=True):
    """f64 inputs, every one exactly representable in f32 (what the kernels are given).  Time-major as the oracle: x [T, N, I],
    keep [T, N]; fused: the loss gradient enters as dheads [T, N, A] through w_head, else as dy [T, N, H]."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s, sc=1.0: (torch.randn(*s, generator=g, dtype=torch.float64) * sc).float().double()
    k = H ** -0.5
    p = {"x": rn(T, N, I), "h0": rn(N, H, sc=0.3), "c0": rn(N, H, sc=0.3), "w_ih": rn(4 * H, I, sc=k), "w_hh": rn(4 * H, H, sc=k),
         "b_ih": rn(4 * H, sc=k), "b_hh": rn(4 * H, sc=k), "dhn": rn(N, H, sc=scale), "dcn": rn(N, H, sc=scale)}
    p["keep"] = None
    if restarts:
        p["keep"] = (torch.rand(T, N, generator=g) > 0.15).double()
        p["keep"][0, 1::2] = 0.0                               # the odd envs restart at step 0: their h0 / c0 get no gradient
    if fused:
        p["w_head"], p["dheads"], p["dy"] = rn(A, H, sc=0.2), rn(T, N, A, sc=scale), None
    else:
        p["w_head"], p["dheads"], p["dy"] = None, None, rn(T, N, H, sc=scale)
    return p


def _reference(p):
    """po.lstm_layer_forward + autograd in f64; results env-major like the kernels'."""
    names = ("x", "h0", "c0", "w_ih", "w_hh", "b_ih", "b_hh") + (("w_head",) if p["dheads"] is not None else ())
    v = {n: p[n].clone().requires_grad_(True) for n in names}
    y, hn, cn = po.lstm_layer_forward(v["x"], v["h0"], v["c0"], v["w_ih"], v["w_hh"], v["b_ih"], v["b_hh"], p["keep"])
    loss = (hn * p["dhn"]).sum() + (cn * p["dcn"]).sum()
    loss = loss + (((y @ v["w_head"].T) * p["dheads"]).sum() if p["dheads"] is not None else (y * p["dy"]).sum())
    loss.backward()
    want = {"y": y.detach().transpose(0, 1), "dx": v["x"].grad.transpose(0, 1), "dw_ih": v["w_ih"].grad, "dw_hh": v["w_hh"].grad,
            "db": v["b_ih"].grad, "dh0": v["h0"].grad, "dc0": v["c0"].grad}
    if p["dheads"] is not None:
        want["dw_head"] = v["w_head"].grad
    return want


def _run(ops, p, need_dx, mode="fp16x3", stash=None):
    """One forward + backward on the GPU under `mode`: fp16x3 (the default: packed gate gradients), dg_f32 (the same step kernels,
    gate gradients kept as f32 rows as well: the round-4 form) or f32_mfma (the generic exact-f32 path; it takes dy only, so a
    fused problem hands it dy = dheads . w_head formed in f64 and the head gradient through wgrad_dheads)."""
    N, T, I = p["x"].shape[1], p["x"].shape[0], p["x"].shape[2]
    d = lambda t: None if t is None else t.float().to(DEV).contiguous()
    tm = lambda t: None if t is None else t.transpose(0, 1)
    xg, kg = d(tm(p["x"])), d(tm(p["keep"]))
    args = [d(p[n]) for n in ("h0", "c0", "w_ih", "w_hh", "b_ih", "b_hh")]
    ops.set_lstm_arith("f32_mfma" if mode == "f32_mfma" else "fp16x3")
    ops.set_debug_flags(*(("dg_f32",) if mode == "dg_f32" else ()))
    try:
        y, _, _, stash = ops.lstm_fwd(xg, kg, *args, stash=stash)
        kw = dict(dhn=d(p["dhn"]), dcn=d(p["dcn"]), need_dx=need_dx)
        if p["dheads"] is None:
            kw["dy"] = d(tm(p["dy"]))
        elif mode == "f32_mfma":
            kw["dy"], kw["wgrad_dheads"] = d(tm(p["dheads"] @ p["w_head"])), d(tm(p["dheads"]))
        else:
            kw["dheads"], kw["w_head"] = d(tm(p["dheads"])), d(p["w_head"])
        g = ops.lstm_bwd(xg, kg, stash, args[2], args[3], y, args[0], **kw)
        g["rows"] = ops.lstm_dgates_f32(g["dgates"], N, T, H)
        torch.cuda.synchronize()
    finally:
        ops.set_lstm_arith("fp16x3")
        ops.set_debug_flags()
    g["y"] = y
    return {k: v.detach().cpu().double() for k, v in g.items() if v is not None and k != "dgates"}


def _errs(got, want):
    """max |got - want| over the largest |want| of each output."""
    return {k: float((got[k] - want[k]).abs().max() / (want[k].abs().max() + 1e-300)) for k in want if k in got}


def _check_bar(e, e_f32, keys, tag):
    """The bar of the h = 128 split-kernel test: f32-level agreement with f64, and no worse than the exact-f32 MFMA chain."""
    for k in keys:
        assert e[k] <= 5e-6, (tag, k, e[k], e)
        assert e[k] <= 2.0 * e_f32[k] + 2e-7, (tag, k, e[k], e_f32[k])


# ------------------------------------------------------------------------------------------------ 1. the dispatch branches
@pytest.mark.parametrize("N,T,I,need_dx,fused", [
    (37, 33, 8, False, True),      # narrow input: dW_ih on the column-sum pass (colsum_pc_kernel)
    (130, 2, 3, False, False),
    (5, 1, 6, False, True),
    (64, 33, 256, False, True),    # hidden-wide input: dW_ih as the second column half of gemm_pc_kernel
    (37, 9, 256, False, False),
    (1, 12, 256, False, True),
    (37, 12, 256, True, False),    # dx formed inside the BPTT's recurrent product, weight gradients still from the pieces
    (5, 33, 40, True, True),       # another width with dx: unpacked to f32 rows, h_prev from y
    (130, 5, 40, False, False),
])
def test_h256_layer_gradients_match_f64(ops, N, T, I, need_dx, fused):
    """Every output of an h = 256 layer -- y, dx where asked, dW_ih, dW_hh, db, dh0, dc0, dW_head -- against an f64 LSTM, for
    shapes that reach each branch of uav_lstm_wgrad's packed path, ragged env counts, T = 1 / 2 / 33, restart masks (odd envs
    restart at step 0), explicit dy and fused dheads + w_head, nonzero dhn / dcn."""
    p = _problem(N, T, I, N * 1000 + T * 10 + I, fused)
    want = _reference(p)
    keys = [k for k in ("y",) + GRADS if k in want and (need_dx or k != "dx")]
    e = _errs(_run(ops, p, need_dx), want)
    e_f32 = _errs(_run(ops, p, need_dx, "f32_mfma"), want)
    _check_bar(e, e_f32, keys, "fp16x3")


# ------------------------------------------------------------------------------------------------ 2. 40 decades
@pytest.mark.parametrize("I", [8, 256])
def test_h256_backward_keeps_f32_accuracy_over_40_decades(ops, I):
    """The per-(env, step) scale of the packed gate gradients exists so that envs whose loss gradients differ by up to 1e25
    (and vary by 1e6 along their own sequence) each come out with f32 relative accuracy: dh0, dc0 and, at I = 256, dx --
    measured per env against an f64 LSTM, relative to that env's own magnitude."""
    N, T = 40, 24
    p = _problem(N, T, I, 4000 + I, fused=True, restarts=False)
    g = torch.Generator().manual_seed(I)
    env_scale = 10.0 ** torch.linspace(-25, 0, N, dtype=torch.float64)
    time_scale = 10.0 ** (-6.0 * torch.rand(T, 1, generator=g, dtype=torch.float64))
    p["dheads"] = (p["dheads"] * env_scale[None, :, None] * time_scale[:, :, None]).float().double()
    p["dhn"] = p["dcn"] = torch.zeros(N, H, dtype=torch.float64)
    want = _reference(p)
    got = _run(ops, p, need_dx=I == H)
    for k in ("dh0", "dc0") + (("dx",) if I == H else ()):
        w_, g_ = want[k].reshape(N, -1), got[k].reshape(N, -1)
        rel = (g_ - w_).abs().amax(1) / w_.abs().amax(1)
        assert float(rel.max()) < 5e-6, (k, rel)
        assert float(w_.abs().amax(1).min()) < 1e-20 < 1e-4 < float(w_.abs().amax(1).max())     # the span is real


# ------------------------------------------------------------------------------------------------ 3. zero gate-gradient rows
def _zero_rows(p, case, N, T):
    """Make (env, step) rows whose gate gradients are exactly zero; returns them as (env, step) pairs."""
    n1, t1 = N // 2, T // 3
    if case == "env":                  # one env without any loss gradient: every row of it is zero
        p["dy"][:, 3] = 0.0
        p["dhn"][3] = p["dcn"][3] = 0.0
        return [(3, t) for t in range(T)]
    src = "dy" if case == "row" else "dheads"
    p[src][t1, n1] = 0.0               # nothing enters at (n1, t1) ...
    p["keep"][t1 + 1, n1] = 0.0        # ... and nothing flows back into it: the episode restarts at t1 + 1
    rows = [(n1, t1)]
    if case == "heads":                # and a last step without gradient (nothing flows back into step T - 1 either)
        p[src][T - 1, 5] = 0.0
        p["dhn"][5] = p["dcn"][5] = 0.0
        rows.append((5, T - 1))
    return rows


@pytest.mark.parametrize("scale", [1e-6, 1.0])
@pytest.mark.parametrize("case", ["env", "row", "heads"])
@pytest.mark.parametrize("N", [64, 37])
@pytest.mark.parametrize("I", [8, 256])
def test_h256_zero_gate_gradient_rows(ops, I, N, case, scale):
    """An (env, step) whose gate gradients are all exactly zero must not set the block scale of the weight-gradient product
    (gemm_pc_kernel scales every h_prev / x row by isc / max isc before the fp16 split): at PPO gradient scale a scale of 1
    from such a row puts the real rows 2^-30 below it, where both fp16 pieces underflow and dW_hh (and dW_ih at I = 256)
    silently collapse to zero while db -- an f32 column sum -- stays right.  dW_hh, dW_ih, db against f64 under the bar
    of the dispatch test, and against the f32-rows form (UAV_DEBUG_DG_F32)."""
    T = 12
    p = _problem(N, T, I, 7000 + N + I, fused=case == "heads", scale=scale)
    rows = _zero_rows(p, case, N, T)
    want = _reference(p)
    got, e_f32 = _run(ops, p, need_dx=False), _errs(_run(ops, p, False, "f32_mfma"), want)
    for n, t in rows:                                          # the rows really are zero
        assert bool((got["rows"][n, t] == 0).all()), (n, t)
    _check_bar(_errs(got, want), e_f32, ("dw_hh", "dw_ih", "db"), (case, scale))
    rows_form = _run(ops, p, need_dx=False, mode="dg_f32")
    for k in ("db", "dw_hh", "dw_ih"):
        err = float((got[k] - rows_form[k]).abs().max())
        assert err <= 2e-6 * float(rows_form[k].abs().max()), (k, err)


@pytest.mark.parametrize("I", [8, 256])
def test_h256_all_zero_gradients_give_zero_weight_gradients(ops, I):
    """No loss gradient at all: every gate-gradient row is zero, and so are the weight gradients -- exactly, not NaN."""
    N, T = 37, 5
    p = _problem(N, T, I, 11, fused=False, scale=0.0)
    got = _run(ops, p, need_dx=False)
    for k in ("dw_hh", "dw_ih", "db", "dh0", "dc0"):
        assert bool((got[k] == 0).all()), (k, got[k].abs().max())


@pytest.mark.parametrize("I", [8, 256])
def test_h256_nan_gradient_is_not_hidden(ops, I):
    """A NaN in one env's dy makes that env's gate gradients NaN from its step back to step 0 (rows that are NaN throughout
    have no finite maximum to scale by).  dW_hh, dW_ih and db must come out non-finite -- as they do in f64 and in the
    f32-rows form -- never as silent zeros; the other envs' dh0 / dc0 stay finite."""
    N, T = 37, 9
    p = _problem(N, T, I, 13, fused=False, scale=1e-6, restarts=False)
    p["dy"][T // 2, 4, 17] = float("nan")
    want = _reference(p)
    for mode in ("fp16x3", "dg_f32"):
        got = _run(ops, p, need_dx=False, mode=mode)
        for k in ("dw_hh", "dw_ih", "db", "dh0", "dc0"):
            assert torch.equal(torch.isfinite(got[k]), torch.isfinite(want[k])), (mode, k, int(torch.isfinite(got[k]).sum()))


# ------------------------------------------------------------------------------------------------ 5. the stash's h_prev slot
@pytest.mark.parametrize("I", [8, 256])
@pytest.mark.parametrize("mode", ["f32_mfma", "dg_f32"])
def test_h256_mode_change_after_forward_is_refused_not_garbage(ops, mode, I):
    """The default h = 256 forward does not write the stash's h_prev slot (the packed weight gradients take h_prev from y).
    If the arithmetic mode or debug flags change between uav_lstm_fwd and the backward, the f32-rows weight gradients would
    read that unwritten slot: the call must be refused, naming the change.  The same problem run in one mode throughout
    (forward again under the new mode, into the same NaN-filled stash) gives dW_hh at f32 accuracy."""
    N, T = 37, 9
    p = _problem(N, T, I, 17, fused=False)
    want = _reference(p)
    d = lambda t: t.float().to(DEV).contiguous()
    tm = lambda t: t.transpose(0, 1)
    xg, kg = d(tm(p["x"])), d(tm(p["keep"]))
    args = [d(p[n]) for n in ("h0", "c0", "w_ih", "w_hh", "b_ih", "b_hh")]
    stash = torch.full((N, T, 6 * H), float("nan"), device=DEV)
    y, _, _, stash = ops.lstm_fwd(xg, kg, *args, stash=stash)          # default mode: the slot stays NaN
    refused, g = None, None
    try:
        if mode == "f32_mfma":
            ops.set_lstm_arith("f32_mfma")
        else:
            ops.set_debug_flags("dg_f32")
        try:
            g = ops.lstm_bwd(xg, kg, stash, args[2], args[3], y, args[0], dy=d(tm(p["dy"])), dhn=d(p["dhn"]), dcn=d(p["dcn"]))
            torch.cuda.synchronize()
        except RuntimeError as ex:
            refused = str(ex)
    finally:
        ops.set_lstm_arith("fp16x3")
        ops.set_debug_flags()
    if refused is None:
        dw = g["dw_hh"].cpu().double()
        pytest.fail(f"mode change not refused: dW_hh all finite {bool(torch.isfinite(dw).all())}, "
                    f"error {_errs({'dw_hh': dw}, want)['dw_hh']:.3g} of its largest f64 element")
    assert "uav_lstm_fwd" in refused and "must not change" in refused, refused
    stash.fill_(float("nan"))
    got = _run(ops, p, need_dx=False, mode=mode, stash=stash)
    e = _errs(got, want)
    assert e["dw_hh"] <= 5e-6, e


@pytest.mark.parametrize("default_steps", [6, 2, 0])
def test_h256_stepper_stash_follows_the_mode_of_every_step(ops, default_steps):
    """The stepper (the h = 256 rollout) writes the stash one step at a time, the h_prev slot only under UAV_DEBUG_DG_F32.
    Steps 0 .. default_steps - 1 under the default flags, the rest under dg_f32, then the backward under dg_f32: refused
    while any step left the slot out; when every step wrote it, dW_hh equals f64."""
    N, T, I = 37, 6, 8
    p = _problem(N, T, I, 19, fused=False)
    want = _reference(p)
    d = lambda t: t.float().to(DEV).contiguous()
    tm = lambda t: t.transpose(0, 1)
    xg, kg = d(tm(p["x"])), d(tm(p["keep"]))
    h0, c0, w_ih, w_hh, b_ih, b_hh = [d(p[n]) for n in ("h0", "c0", "w_ih", "w_hh", "b_ih", "b_hh")]
    y, stash = torch.zeros(N, T, H, device=DEV), torch.full((N, T, 6 * H), float("nan"), device=DEV)
    sp = ops.LstmStepper(N, I, H, DEV)
    refused, g = None, None
    try:
        sp.begin(w_ih, w_hh, b_ih, b_hh, h0, c0)
        for t in range(T):
            if t == default_steps:
                ops.set_debug_flags("dg_f32")
            sp.step(xg, t, y, stash, keep=kg[:, t].contiguous())
        ops.set_debug_flags("dg_f32")
        try:
            g = ops.lstm_bwd(xg, kg, stash, w_ih, w_hh, y, h0, dy=d(tm(p["dy"])), dhn=d(p["dhn"]), dcn=d(p["dcn"]))
            torch.cuda.synchronize()
        except RuntimeError as ex:
            refused = str(ex)
    finally:
        ops.set_debug_flags()
    if default_steps > 0:
        assert refused is not None and "must not change" in refused, refused
    else:
        assert refused is None, refused
        assert _errs({"dw_hh": g["dw_hh"].cpu().double()}, want)["dw_hh"] <= 5e-6
