"""Record tests/golden/h256_bits.json: SHA-256 digests of what the h = 256 fp16-split step path writes.

The step kernels of csrc/lstm_h3.hip (one launch per time step: sequence forward, stepper, BPTT, the pipelined BPTT of a stack) and
the weight-gradient pass that reads their piece chunks (csrc/wgrad_pc.hip) are what the C5 configuration runs, and what gets tuned
next: how the host lays out its workspace, which launches it issues and how a kernel forms its addresses may change, what lands in
the output buffers must not.  tests/test_gpu_h256_bits.py compares every output buffer of the cases below with the digests recorded
here -- by the build BEFORE such a change, on the GPU:

    UAVPPO_LIB=/path/to/the/parent/build/libuavppo.so python tools/gen_golden_h256_bits.py [OUT]

(UAVPPO_LIB selects the library; without it the tree's own build records.)  Every case runs twice and nothing is written when two
runs differ.  Inputs come from numpy's RandomState; nothing outside the repository is read.  All cases run on the default fp16-split
arithmetic, restart masks with several zeros per sequence:

    fwd (N, T, I) = (5, 6, 6)       one ragged tile, one input slab, x gathered as f32 rows
                    (37, 3, 40)     two input slabs with a ragged second one
                    (70, 2, 256)    two env tiles, eight slabs: x staged as piece planes (split_x_kernel), one chunk
                    (33, 20, 256)   more than one 16-step chunk of staged x
    bwd             uav_lstm_fwd + uav_lstm_bwd + uav_lstm_wgrad of one layer: (33, 4, 256) with dx (formed in the BPTT's recurrent
                    product) and without (dheads + w_head), (5, 6, 6) on the narrow weight-gradient pass
    stack           uav_lstm_bwd_stack of two layers at N = 33, T = 4 (I = 8 below, 256 above), then both layers' weight gradients
    stepper, pair   the two-layer stepper loop at (80, 5, 8), the upper layer reading the lower one's piece planes -- layer by layer,
                    and with layer 1's step t + 1 beside layer 2's step t in one launch (uav_lstm_stepper_step_pair)
    dgf32           (33, 4, 256) under the dg_f32 debug flag: gate gradients as f32 rows, the stash's h_prev slot written

A buffer is digested whole where the path writes all of it; of the stash only the slots that belong to the contract (the h_prev slot
under dg_f32 alone).  Gate gradients are digested as the rows uav_lstm_dgates_f32 returns and, in the packed form, as the raw
zero-initialised buffer too.
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
PATH = os.path.join(ROOT, "tests", "golden", "h256_bits.json")
H, NHD = 256, 6
FWD_SHAPES = ((5, 6, 6), (37, 3, 40), (70, 2, 256), (33, 20, 256))


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _uni(rs, shape, bound):
    return rs.uniform(-bound, bound, size=shape).astype(np.float32)


def _keep(rs, N, T):
    """restart masks: about one step in six restarts, every sequence has a zero, env 0 restarts at t = 0"""
    k = (rs.uniform(size=(N, T)) > 1.0 / 6.0).astype(np.float32)
    k[np.arange(N), rs.randint(0, T, size=N)] = 0.0
    k[0, 0] = 0.0
    return k


def layer_inputs(N, T, I, seed):
    rs = np.random.RandomState(seed)
    b = 1.0 / np.sqrt(H)
    return {"x": _uni(rs, (N, T, I), 2.0), "keep": _keep(rs, N, T), "h0": _uni(rs, (N, H), 0.5), "c0": _uni(rs, (N, H), 0.5),
            "w_ih": _uni(rs, (4 * H, I), b), "w_hh": _uni(rs, (4 * H, H), b), "b_ih": _uni(rs, 4 * H, b), "b_hh": _uni(rs, 4 * H, b),
            "w_head": _uni(rs, (NHD, H), 3 * b), "dy": (rs.randn(N, T, H) * 1e-3).astype(np.float32),
            "dheads": (rs.randn(N, T, NHD) * 1e-2).astype(np.float32), "dhn": (rs.randn(N, H) * 1e-3).astype(np.float32),
            "dcn": (rs.randn(N, H) * 1e-3).astype(np.float32)}


def _fwd(ops, d, whole_stash=False):
    """uav_lstm_fwd into zeroed buffers -> (y, stash, {name: tensor to digest})"""
    N, T, _ = d["x"].shape
    stash = torch.zeros(N, T, 6 * H, device=DEV)
    y, hn, cn, stash = ops.lstm_fwd(d["x"], d["keep"], d["h0"], d["c0"], d["w_ih"], d["w_hh"], d["b_ih"], d["b_hh"], stash=stash,
                                    y=torch.zeros(N, T, H, device=DEV))
    return y, stash, {"y": y, "hn": hn, "cn": cn, "stash": stash if whole_stash else stash[..., :5 * H]}


def run_fwd(N, T, I):
    from uavppo import ops
    d = {k: _dev(v) for k, v in layer_inputs(N, T, I, 100 * N + 10 * T + I).items()}
    return _fwd(ops, d)[2]


def _grads(ops, g, N, T, prefix=""):
    out = {prefix + k: g[k] for k in ("dx", "dw_ih", "dw_hh", "db", "dh0", "dc0", "dw_head") if g.get(k) is not None}
    out[prefix + "dgates_rows"] = ops.lstm_dgates_f32(g["dgates"], N, T, H)
    return out


def run_bwd(N, T, I, need_dx, fused, flags=()):
    """one layer: forward, BPTT, weight gradients; fused: the loss gradient enters as dheads through w_head, else as dy"""
    from uavppo import ops
    d = {k: _dev(v) for k, v in layer_inputs(N, T, I, 7 + 100 * N + 10 * T + I).items()}
    ops.set_debug_flags(*flags)
    try:
        y, stash, out = _fwd(ops, d, whole_stash="dg_f32" in flags)
        dgates = ops.lstm_dgates(N, T, H, DEV).zero_()
        kw = dict(dheads=d["dheads"], w_head=d["w_head"]) if fused else dict(dy=d["dy"])
        g = ops.lstm_bwd(d["x"], d["keep"], stash, d["w_ih"], d["w_hh"], y, d["h0"], dhn=d["dhn"], dcn=d["dcn"], need_dx=need_dx,
                         dgates=dgates, **kw)
        out.update(_grads(ops, g, N, T))
        if "dg_f32" not in flags:
            out["dgates_raw"] = dgates
        torch.cuda.synchronize()
    finally:
        ops.set_debug_flags()
    return out


def run_stack(N, T):
    """two layers (I = 8 below, 256 above): forwards, uav_lstm_bwd_stack top first, then each layer's weight gradients"""
    from uavppo import ops
    lo = {k: _dev(v) for k, v in layer_inputs(N, T, 8, 11 + 100 * N + T).items()}
    hi = {k: _dev(v) for k, v in layer_inputs(N, T, H, 13 + 100 * N + T).items()}
    hi["keep"] = lo["keep"]
    y0, st0, _ = _fwd(ops, lo)
    hi["x"] = y0
    y1, st1, _ = _fwd(ops, hi)
    dg0, dg1 = ops.lstm_dgates(N, T, H, DEV).zero_(), ops.lstm_dgates(N, T, H, DEV).zero_()
    dx1 = torch.zeros(N, T, H, device=DEV)
    ops.lstm_bwd_stack([{"stash": st1, "w_hh": hi["w_hh"], "w_ih": hi["w_ih"], "dgates": dg1, "dx": dx1},
                        {"stash": st0, "w_hh": lo["w_hh"], "dgates": dg0}], lo["keep"], dheads=hi["dheads"], w_head=hi["w_head"])
    g1 = ops.lstm_bwd(y0, lo["keep"], st1, hi["w_ih"], hi["w_hh"], y1, hi["h0"], dgates=dg1, bwd_done=True, want_dstate=False,
                      wgrad_dheads=hi["dheads"])
    g0 = ops.lstm_bwd(lo["x"], lo["keep"], st0, lo["w_ih"], lo["w_hh"], y0, lo["h0"], dgates=dg0, bwd_done=True, want_dstate=False)
    out = {"l1.dx": dx1, "l0.dgates_raw": dg0, "l1.dgates_raw": dg1}
    out.update(_grads(ops, g1, N, T, "l1."))
    out.update(_grads(ops, g0, N, T, "l0."))
    torch.cuda.synchronize()
    return out


def run_stepper(N, T, I, pairs):
    """the two-layer stepper loop, layer 2 on layer 1's piece planes; pairs: layer 1's step t + 1 beside layer 2's step t"""
    from uavppo import ops
    lo = {k: _dev(v) for k, v in layer_inputs(N, T, I, 17 + 100 * N + 10 * T + I).items()}
    hi = {k: _dev(v) for k, v in layer_inputs(N, T, H, 19 + 100 * N + 10 * T + I).items()}
    keep = lo["keep"].t().contiguous()
    sp = [ops.LstmStepper(N, I, H, DEV), ops.LstmStepper(N, H, H, DEV)]
    for s, d in zip(sp, (lo, hi)):
        s.hn.zero_()
        s.cn.zero_()
        s.begin(d["w_ih"], d["w_hh"], d["b_ih"], d["b_hh"], d["h0"], d["c0"])
    y = [torch.zeros(N, T, H, device=DEV) for _ in range(2)]
    st = [torch.zeros(N, T, 6 * H, device=DEV) for _ in range(2)]
    x = lo["x"]
    if pairs:
        sp[0].step(x, 0, y[0], st[0], keep=keep[0])
        for t in range(T - 1):
            ops.lstm_stepper_step_pair((sp[0], x, t + 1, y[0], st[0], None, keep[t + 1]), (sp[1], y[0], t, y[1], st[1], sp[0], keep[t]))
        sp[1].step(y[0], T - 1, y[1], st[1], below=sp[0], keep=keep[T - 1])
    else:
        for t in range(T):
            sp[0].step(x, t, y[0], st[0], keep=keep[t])
            sp[1].step(y[0], t, y[1], st[1], below=sp[0], keep=keep[t])
    torch.cuda.synchronize()
    out = {}
    for l in range(2):
        out.update({f"l{l}.y": y[l], f"l{l}.stash": st[l][..., :5 * H], f"l{l}.hn": sp[l].hn, f"l{l}.cn": sp[l].cn})
    return out


def cases():
    """name -> callable() -> {buffer name: tensor}"""
    c = {"fwd-n%d-t%d-i%d" % s: (lambda s=s: run_fwd(*s)) for s in FWD_SHAPES}
    c["bwd-n33-t4-i256-dx"] = lambda: run_bwd(33, 4, 256, True, False)
    c["bwd-n33-t4-i256-nodx"] = lambda: run_bwd(33, 4, 256, False, True)
    c["bwd-n5-t6-i6"] = lambda: run_bwd(5, 6, 6, False, True)
    c["stack-n33-t4"] = lambda: run_stack(33, 4)
    c["stepper-n80-t5-i8"] = lambda: run_stepper(80, 5, 8, False)
    c["pair-n80-t5-i8"] = lambda: run_stepper(80, 5, 8, True)
    c["dgf32-n33-t4-i256"] = lambda: run_bwd(33, 4, 256, True, False, flags=("dg_f32",))
    return c


def run_case(name):
    from uavppo import ops
    with ops.lstm_arith("fp16x3"):
        return {k: _sha(v) for k, v in cases()[name]().items()}


def main():
    out, unstable = {}, []
    for name in cases():
        out[name] = run_case(name)
        again = run_case(name)
        unstable += [f"{name}.{k}" for k in out[name] if again[k] != out[name][k]]
        print(f"{name}: {len(out[name])} buffers")
    if unstable:
        raise SystemExit("two runs differ, nothing written: " + ", ".join(unstable))
    path = sys.argv[1] if len(sys.argv) > 1 else PATH
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{path}: {len(out)} cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
