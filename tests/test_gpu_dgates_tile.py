"""Tile form of the h = 64 / 128 gate gradients (include/uavppo.h, uav_lstm_dgates_tile; csrc/lstm_forms.h DgTile): the BPTT writes the
16 rows of a workgroup's step as one contiguous block, the weight-gradient pass reads them there.  Nothing but the place of a row
changes, so everything is held to BIT equality with the f32-rows form of the same call: the gate gradients themselves (through
uav_lstm_dgates_f32), dh0 / dc0, every weight gradient, and a trainer's parameters, Adam moments and loss sums after three iterations.
Shapes: one tile, a ragged last tile, several tiles (a weight-gradient workgroup then starts inside an env), T a multiple of 32 but
not of 64; with and without restart masks; both split arithmetics.  The form is opt-in per buffer and per call: whoever does not
ask gets f32 rows, and a buffer is refused by uav_lstm_wgrad when what it holds is not what the call would read.
Every test drops the records it made (lstm_dgates_forget): the device handle is shared with the tests that run after it.
-m gpu."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NHD = 6
SHAPES = [(16, 32), (17, 32), (33, 64), (48, 96)]
CASES = [(H, N, T, masks, arith) for H in (64, 128) for N, T in SHAPES for masks in (False, True) for arith in ("fp16x3", "bf16x6")]
IDS = ["h%d-%dx%d-%s-%s" % (H, N, T, "masks" if m else "nomasks", a) for H, N, T, m, a in CASES]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(None)
def _inputs(H, N, T, masks, I=6):
    """parameters at nn.LSTM's scale, observations, a start state and head gradients; the forward pass that fills stash and y is the
    library's own (its results are inputs here, the same for both forms)"""
    rs = np.random.RandomState(7 * H + 131 * N + T + (1 if masks else 0) + 1000 * I)
    b = 1.0 / np.sqrt(H)
    u = lambda *shape, bound=b: rs.uniform(-bound, bound, size=shape).astype(np.float32)     # noqa: E731
    keep = np.ones((N, T), np.float32)
    if masks:                                   # about one step in six restarts; env 0 restarts at t = 0, the last env at the last step
        keep = (rs.uniform(size=(N, T)) > 1.0 / 6.0).astype(np.float32)
        keep[0, 0] = 0.0
        keep[N - 1, T - 1] = 0.0
    return {k: _dev(v) for k, v in dict(
        x=u(N, T, I, bound=2.0), keep=keep, h0=u(N, H, bound=1.0), c0=u(N, H, bound=1.0), w_ih=u(4 * H, I), w_hh=u(4 * H, H),
        b_ih=u(4 * H), b_hh=u(4 * H), w_head=u(NHD, H), b_head=u(NHD), dheads=(rs.randn(N, T, NHD) * 1e-2).astype(np.float32),
        dhn=u(N, H, bound=1e-2), dcn=u(N, H, bound=1e-2)).items()}


def _backward(H, N, T, masks, arith, tile, I=6, dgates=None):
    """ops.lstm_bwd (BPTT + weight gradients) on the rows form (the library's own allocation) or on a tile-form buffer"""
    from uavppo import ops
    p = _inputs(H, N, T, masks, I)
    with ops.lstm_arith(arith):
        y, _, _, stash = ops.lstm_fwd(p["x"], p["keep"], p["h0"], p["c0"], p["w_ih"], p["w_hh"], p["b_ih"], p["b_hh"])
        if tile and dgates is None:
            dgates = ops.lstm_dgates_tile(N, T, I, H, DEV)
            assert dgates is not None, ops.lib().uav_last_error()
            dgates.fill_(float("nan"))          # rows of a ragged last tile that nobody writes must not be read either
        r = ops.lstm_bwd(p["x"], p["keep"], stash, p["w_ih"], p["w_hh"], y, p["h0"], dheads=p["dheads"], w_head=p["w_head"],
                         dhn=p["dhn"], dcn=p["dcn"], dgates=dgates, dgates_tile=tile)
        r["rows"] = ops.lstm_dgates_f32(r["dgates"], N, T, H)
    r["y"], r["stash"] = y, stash
    torch.cuda.synchronize()
    return r


@pytest.mark.parametrize("H,N,T,masks,arith", CASES, ids=IDS)
def test_tile_form_is_bit_identical_to_rows(H, N, T, masks, arith):
    from uavppo import ops
    rows = _backward(H, N, T, masks, arith, False)
    assert ops.lstm_dgates_form(rows["dgates"]) == ops.DG_ROWS and rows["dgates"].shape == (N, T, 4 * H)
    assert torch.equal(rows["rows"], rows["dgates"])
    assert torch.isfinite(rows["rows"]).all() and float(rows["rows"].abs().max()) > 0
    tile = _backward(H, N, T, masks, arith, True)
    try:
        assert ops.lstm_dgates_form(tile["dgates"]) == ops.DG_TILE
        # 1. the gate gradients, returned as rows, and the start-state gradients
        assert torch.equal(tile["rows"], rows["rows"])
        assert torch.equal(tile["dh0"], rows["dh0"]) and torch.equal(tile["dc0"], rows["dc0"])
        # ... and they lie where the header says: element (n, t, c) at (((n / 16) T + t) 16 + n % 16) 4H + c
        n, t = torch.meshgrid(torch.arange(N, device=DEV), torch.arange(T, device=DEV), indexing="ij")
        at = ((n // 16) * T + t) * 16 + n % 16
        assert torch.equal(tile["dgates"].view(-1, 4 * H)[at], rows["rows"])
        # 2. the weight gradients
        for k in ("dw_hh", "dw_ih", "db", "dw_head"):
            assert torch.isfinite(rows[k]).all() and torch.equal(tile[k], rows[k]), k
        # the weight-gradient pass alone, with and without the head tile, reads the recorded form as well
        p = _inputs(H, N, T, masks)
        with ops.lstm_arith(arith):
            for dh in (p["dheads"], None):
                a = ops.lstm_wgrad(p["x"], p["keep"], p["h0"], rows["y"], rows["stash"], rows["dgates"], p["w_ih"], dheads=dh)
                b = ops.lstm_wgrad(p["x"], p["keep"], p["h0"], tile["y"], tile["stash"], tile["dgates"], p["w_ih"], dheads=dh)
                for k in a:
                    assert (a[k] is None and b[k] is None) or torch.equal(a[k], b[k]), (k, dh is None)
        # one arming serves one call: the next BPTT on the same buffer that does not ask writes rows again
        again = _backward(H, N, T, masks, arith, False, dgates=tile["dgates"])
        assert ops.lstm_dgates_form(again["dgates"]) == ops.DG_ROWS
        assert torch.equal(again["dgates"].view(-1)[:N * T * 4 * H].view(N, T, 4 * H), rows["rows"])
        assert torch.equal(again["dw_hh"], rows["dw_hh"])
    finally:
        ops.lstm_dgates_forget(tile["dgates"])


@pytest.mark.parametrize("H,N,T,masks,arith", CASES, ids=IDS)
def test_wgrad_refuses_a_buffer_of_the_other_form(H, N, T, masks, arith):
    """3.: as at h = 256, uav_lstm_wgrad does not read a buffer as something it was not written as"""
    from uavppo import ops
    p = _inputs(H, N, T, masks)
    tile = _backward(H, N, T, masks, arith, True)
    rows = _backward(H, N, T, masks, arith, False, dgates=ops.lstm_dgates_tile(N, T, 6, H, DEV))
    wgrad = lambda r, **kw: ops.lstm_wgrad(kw.get("x", p["x"]), kw.get("keep", p["keep"]), p["h0"], kw.get("y", r["y"]),     # noqa: E731
                                           kw.get("stash", r["stash"]), r["dgates"], p["w_ih"])
    try:
        # tile blocks, but the exact-f32 kernels read rows only
        with ops.lstm_arith("f32_mfma"), pytest.raises(RuntimeError, match="tile form"):
            wgrad(tile)
        # tile blocks of (N, T), read as (N, T / 2)
        h = T // 2
        with ops.lstm_arith(arith), pytest.raises(RuntimeError, match="tile form"):
            wgrad(tile, x=p["x"][:, :h].contiguous(), keep=p["keep"][:, :h].contiguous(), y=tile["y"][:, :h].contiguous(),
                  stash=tile["stash"][:, :h].contiguous())
        # f32 rows in a buffer that is (only) armed for tile form
        ops._arm_tile(rows["dgates"], N, T, 6, H)
        assert ops.lstm_dgates_form(rows["dgates"]) == ops.DG_TILE_ARMED
        with ops.lstm_arith(arith):
            with pytest.raises(RuntimeError, match="armed"):
                wgrad(rows)
            with pytest.raises(RuntimeError, match="armed"):
                ops.lstm_dgates_f32(rows["dgates"], N, T, H)
            ops.lstm_dgates_forget(rows["dgates"])
            assert torch.equal(wgrad(rows)["dw_hh"], tile["dw_hh"])          # forgotten: rows again, and the same sums
    finally:
        ops.lstm_dgates_forget(tile["dgates"])
        ops.lstm_dgates_forget(rows["dgates"])


@pytest.mark.parametrize("H", [64, 128])
def test_shapes_without_tile_form_are_refused_and_run_on_rows(H):
    """4.: T = 40 is no multiple of the weight-gradient kernels' 32-row slab, I = 8 takes the generic weight-gradient products"""
    from uavppo import ops
    from uavppo.trainer import VecPPOTrainer
    N = 32
    for T, I, why in ((40, 6, "multiple of 32"), (32, 8, "at most 6")):
        assert ops.lstm_dgates_tile_bytes(N, T, I, H, DEV) == 0 and ops.lstm_dgates_tile(N, T, I, H, DEV) is None
        assert why in ops.lib().uav_last_error().decode()
        buf = torch.empty(2 * N * T * 4 * H, device=DEV)
        with pytest.raises(RuntimeError, match=why):
            _backward(H, N, T, True, "fp16x3", True, I=I, dgates=buf)
        assert ops.lstm_dgates_form(buf) == ops.DG_ROWS
        r = _backward(H, N, T, True, "fp16x3", False, I=I, dgates=buf)
        own = _backward(H, N, T, True, "fp16x3", False, I=I)
        assert ops.lstm_dgates_form(buf) == ops.DG_ROWS and torch.isfinite(r["rows"]).all()
        assert torch.equal(r["rows"], own["rows"]) and torch.equal(r["dw_hh"], own["dw_hh"]) and torch.equal(r["dw_ih"], own["dw_ih"])
    assert ops.lstm_dgates_tile_bytes(N, 32, 6, 256, DEV) == 0                     # h = 256 has its own form
    with ops.lstm_arith("f32_mfma"):
        assert ops.lstm_dgates_tile_bytes(N, 32, 6, H, DEV) == 0
    assert ops.lstm_dgates_tile_bytes(17, 32, 6, H, DEV) == 32 * 32 * 4 * H * 4     # padded to whole tiles
    # a trainer that asks for the form at such a shape keeps rows and trains
    for kw in (dict(horizon=40), dict(horizon=32, trend_k=2)):
        tr = VecPPOTrainer(N, policy="lstm", hidden=H, device=DEV, seed=5, use_curriculum=False, epochs=2, dgates_tile=True, **kw)
        assert tr.policy.dgates_tile is False
        tr.train_iteration()
        assert all(np.isfinite(tr.losses())) and ops.lstm_dgates_form(tr.work["dgates"]) == ops.DG_ROWS


def test_a_handle_keeps_eight_records_and_evicts_none():
    from uavppo import ops
    bufs = [ops.lstm_dgates_tile(16, 32, 6, 64, DEV) for _ in range(9)]
    try:
        for b in bufs[:8]:
            ops._arm_tile(b, 16, 32, 6, 64)
        with pytest.raises(RuntimeError, match="forget"):
            ops._arm_tile(bufs[8], 16, 32, 6, 64)
        assert [ops.lstm_dgates_form(b) for b in bufs] == [ops.DG_TILE_ARMED] * 8 + [ops.DG_ROWS]
        ops.lstm_dgates_forget(bufs[0])
        ops._arm_tile(bufs[8], 16, 32, 6, 64)
        ops._arm_tile(bufs[8], 16, 32, 6, 64)                                   # arming again reuses the buffer's own record
    finally:
        for b in bufs:
            ops.lstm_dgates_forget(b)
    assert all(ops.lstm_dgates_form(b) == ops.DG_ROWS for b in bufs)


def test_a_buffer_has_one_record_through_pieces_tile_and_forget():
    """One buffer, three writers in a row: an h = 256 BPTT (fp16 piece chunks), an armed h = 64 BPTT (tile blocks), then forget.
    The handle keeps ONE record per buffer (csrc/lstm_forms.h), so what it reports is always the last of them -- after the forget
    f32 rows, not the pieces of two calls ago."""
    from uavppo import ops
    N, T, H = 16, 32, 64
    N2, T2, H2 = 5, 1, 256                      # the smallest piece-form shape of tests/test_gpu_lstm_h256.py
    buf = ops.lstm_dgates_tile(N, T, 6, H, DEV)
    assert buf is not None and buf.numel() * 4 >= ops.lstm_dgates_bytes(N2, T2, H2, DEV)
    try:
        p = _inputs(H2, N2, T2, False)
        with ops.lstm_arith("fp16x3"):
            y, _, _, stash = ops.lstm_fwd(p["x"], p["keep"], p["h0"], p["c0"], p["w_ih"], p["w_hh"], p["b_ih"], p["b_hh"])
            ops.lstm_bwd(p["x"], p["keep"], stash, p["w_ih"], p["w_hh"], y, p["h0"], dheads=p["dheads"], w_head=p["w_head"],
                         dhn=p["dhn"], dcn=p["dcn"], dgates=buf)
        assert ops.lstm_dgates_form(buf) == ops.DG_PIECES
        rows = _backward(H, N, T, False, "fp16x3", False)
        tile = _backward(H, N, T, False, "fp16x3", True, dgates=buf)
        assert ops.lstm_dgates_form(buf) == ops.DG_TILE
        for k in ("dw_hh", "dw_ih", "db", "dw_head"):
            assert torch.isfinite(rows[k]).all() and torch.equal(tile[k], rows[k]), k
        ops.lstm_dgates_forget(buf)
        assert ops.lstm_dgates_form(buf) == ops.DG_ROWS
    finally:
        ops.lstm_dgates_forget(buf)


def _train(tile, N=64, T=32, H=64, iters=3, **kw):
    from uavppo.trainer import VecPPOTrainer
    tr = VecPPOTrainer(N, T, "lstm", hidden=H, device=DEV, seed=11, use_curriculum=False, dgates_tile=tile, **kw)
    assert tr.policy.dgates_tile is tile
    tr.record = True
    for _ in range(iters):
        tr.train_iteration()
    torch.cuda.synchronize()
    return tr


def _same_training(a, b):
    assert a.opt_step == b.opt_step and len(a.log) == len(b.log) > 0
    for name in ("flat",):
        assert torch.equal(getattr(a.policy, name), getattr(b.policy, name)), name
    assert torch.equal(a.exp_avg, b.exp_avg) and torch.equal(a.exp_avg_sq, b.exp_avg_sq)
    for (la, ga), (lb, gb) in zip(a.log, b.log):
        assert la.cpu().numpy().tobytes() == lb.cpu().numpy().tobytes() and ga.cpu().numpy().tobytes() == gb.cpu().numpy().tobytes()
    assert torch.isfinite(a.policy.flat).all()


def test_trainer_is_byte_identical_with_the_form_on_and_off():
    """5.: 64 x 32, h = 64, three iterations"""
    from uavppo import ops
    on, off = _train(True), _train(False)
    _same_training(on, off)
    # the request is per call and leaves nothing behind on the shared handle
    assert ops.lstm_dgates_form(on.work["dgates"]) == ops.DG_ROWS


def test_trainer_rule_and_minibatches():
    """the default asks for the form only where every CU has a tile (C3: 256 tiles; not at 64 envs), and the form follows the
    minibatch shape the update's kernels are handed, ragged last tile included"""
    from uavppo.trainer import VecPPOTrainer
    tr = VecPPOTrainer(64, 32, "lstm", hidden=64, device=DEV, seed=11, use_curriculum=False)
    assert tr.policy.dgates_tile is False
    kw = dict(N=72, num_minibatches=3, shuffle_envs=True, iters=2)               # minibatches of 24 envs: 1.5 tiles
    _same_training(_train(True, **kw), _train(False, **kw))
