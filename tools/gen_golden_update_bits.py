"""Record tests/golden/update_bits.json: SHA-256 digests of what the h = 64 / 128 update kernels write.

lstm_fwd_split (csrc/lstm.hip) and lstm_wgrad_split (csrc/wgrad.hip) are bound by instruction issue and get tuned for it: how they
form their addresses and stage their inputs may change, what they compute must not.  tests/test_gpu_update_bits.py compares every output
buffer of the cases below with the digests recorded here -- by the build BEFORE such a change, on the GPU:

    python tools/gen_golden_update_bits.py [OUT]    # at the parent commit of the change; OUT defaults to the golden file

and, so that a wrong address fails even against a regenerated recording, with an f64 restatement (want_wgrad / want_fwd below).
Inputs come from numpy's RandomState; nothing outside the repository is read.

Weight gradients (uav_lstm_wgrad from given gate gradients), H in {64, 128}, with and without dheads, keep with several zeros per
sequence:
    N = 256, T = 96   three 32-row slabs per workgroup on 256 workgroups; sequence starts fall at different rows of the 8-row
                      groups: the prefetch's tail clamp and the t == 0 / h0 row inside the slab loop
    N = 48, T = 40    one slab per workgroup on 60 workgroups: the clamp applies to every prefetch
    N = 20, T = 8     five single-slab workgroups, a sequence start in every 8-row group
    N = 20, T = 9     180 rows are no whole number of 32-row slabs: the exact-f32 kernel (lstm_wgrad_kernel), which must stay as it is
Forward (uav_lstm_fwd), H in {64, 128}, T in {8, 9, 17, 40} (one chunk of 8 steps; a one-step tail chunk; three chunks; five),
N in {16, 20} (a full tile of 16 envs; a second tile with 12 dead env lanes), every combination of stash / heads / keep given or not
and I = 6 or 3 (padding features), plus the form that reads its input projection from the stash (I = 16).
BPTT + weight gradients (uav_lstm_bwd + uav_lstm_wgrad on the stash and y of run_fwd in the same arithmetic), H in {64, 128}, I = 6, keep,
non-zero dhn / dcn, (N, T) in {(16, 8), (20, 9), (20, 40)} (a full tile; a second tile with 12 dead env lanes and an odd T; several
staging chunks), driven once by dheads + w_head (the split BPTT) and once by plain dy (the exact-f32 lstm_bwd_kernel in every
arithmetic): the gate gradients as f32 rows, dh0, dc0 and every weight gradient.  (N, T) = (20, 32) once more with the gate gradients
in tile form (the _tile kernels' own bits).
Every case above runs on fp16x3.  A case whose name ends in -bf16x6 or -f32_mfma runs on that arithmetic: the forward at T in {9, 17},
N = 20 (i6-stash-heads-keep and i16), the BPTT at (20, 9), the weight gradients at (48, 40) and (20, 8).
"""
import hashlib
import itertools
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
PATH = os.path.join(ROOT, "tests", "golden", "update_bits.json")
WGRAD_SHAPES = ((256, 96), (48, 40), (20, 8), (20, 9))
FWD_T, FWD_N = (8, 9, 17, 40), (16, 20)
BWD_SHAPES, BWD_TILE_SHAPE = ((16, 8), (20, 9), (20, 40)), (20, 32)
ARITHS = ("fp16x3", "bf16x6", "f32_mfma")
OTHER_FWD_T, OTHER_FWD_N, OTHER_BWD_SHAPE, OTHER_WGRAD_SHAPES = (9, 17), 20, (20, 9), ((48, 40), (20, 8))
OTHER_FWD_COMBOS = ((6, True, True, True), (16, True, True, True), (16, True, False, True))
BWD_DRIVES = ("heads", "dy")
NHD = 6


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _uni(rs, shape, bound):
    return rs.uniform(-bound, bound, size=shape).astype(np.float32)


def _keep(rs, N, T):
    """restart masks: about one step in six restarts, and every sequence has at least two zeros (one of them at t = 0 for env 0)"""
    k = (rs.uniform(size=(N, T)) > 1.0 / 6.0).astype(np.float32)
    k[np.arange(N), rs.randint(0, T, size=N)] = 0.0
    k[np.arange(N), rs.randint(0, T, size=N)] = 0.0
    k[0, 0] = 0.0
    return k


# ------------------------------------------------------------------------------------------------ weight gradients
def wgrad_inputs(H, N, T):
    rs = np.random.RandomState(1000 * H + 10 * N + T)
    return {"x": _uni(rs, (N, T, 6), 2.0), "keep": _keep(rs, N, T), "h0": _uni(rs, (N, H), 1.0), "y": _uni(rs, (N, T, H), 1.0),
            "dgates": (rs.randn(N, T, 4 * H) * 1e-3).astype(np.float32), "dheads": (rs.randn(N, T, NHD) * 1e-2).astype(np.float32)}


def run_wgrad(inp, heads, arith="fp16x3"):
    """{dw_ih, dw_hh, db[, dw_head]} of uav_lstm_wgrad on the arithmetic `arith`"""
    from uavppo import ops
    N, T, H = inp["y"].shape
    stash = torch.zeros(N, T, 6 * H, device=DEV)                         # the I <= 6 path does not read it
    with ops.lstm_arith(arith):
        g = ops.lstm_wgrad(_dev(inp["x"]), _dev(inp["keep"]), _dev(inp["h0"]), _dev(inp["y"]), stash, _dev(inp["dgates"]),
                           torch.zeros(4 * H, 6, device=DEV), dheads=_dev(inp["dheads"]) if heads else None)
    torch.cuda.synchronize()
    return {k: v for k, v in g.items() if v is not None}


def want_wgrad(inp, heads):
    """the same sums in f64, from the f32 values the kernel is given"""
    d = {k: torch.from_numpy(v).double() for k, v in inp.items()}
    hprev = torch.cat([d["h0"][:, None], d["y"][:, :-1]], 1) * d["keep"][..., None]
    out = {"dw_hh": torch.einsum("ntm,ntu->mu", d["dgates"], hprev), "dw_ih": torch.einsum("ntm,nti->mi", d["dgates"], d["x"]),
           "db": d["dgates"].sum((0, 1))}
    if heads:
        out["dw_head"] = torch.einsum("nta,ntu->au", d["dheads"], d["y"])
    return out


# ------------------------------------------------------------------------------------------------ forward
def fwd_combos():
    """(I, stash, heads, keep) of one (H, T, N) case: all sixteen fused forms at I = 6 and at I = 3, and the unfused form"""
    c = [(I, s, h, k) for I in (6, 3) for s, h, k in itertools.product((True, False), repeat=3)]
    return c + [(16, True, h, True) for h in (True, False)]


def combo_name(I, stash, heads, keep):
    return "i%d-%s-%s-%s" % (I, "stash" if stash else "nostash", "heads" if heads else "noheads", "keep" if keep else "nokeep")


def fwd_inputs(H, T, N, I):
    rs = np.random.RandomState(1000 * H + 10 * T + N + 7 * I)
    b = 1.0 / np.sqrt(H)
    return {"x": _uni(rs, (N, T, I), 2.0), "keep": _keep(rs, N, T), "h0": _uni(rs, (N, H), 0.5), "c0": _uni(rs, (N, H), 0.5),
            "w_ih": _uni(rs, (4 * H, I), b), "w_hh": _uni(rs, (4 * H, H), b), "b_ih": _uni(rs, 4 * H, b), "b_hh": _uni(rs, 4 * H, b),
            "w_head": _uni(rs, (NHD, H), 3 * b), "b_head": _uni(rs, NHD, 0.5)}


def run_fwd(inp, stash, heads, keep, arith="fp16x3", whole_stash=False):
    """{y, hn, cn[, stash][, heads]} of uav_lstm_fwd.  Of the stash rows the gates and c_prev are always part of the contract, the
    h_prev slot only where the kernel writes it (I > 6); whole_stash: the buffer as it is, for the BPTT to read."""
    from uavppo import ops
    N, T, I = inp["x"].shape
    hb = torch.full((N, T, NHD), float("nan"), device=DEV) if heads else None
    with ops.lstm_arith(arith):
        y, hn, cn, st = ops.lstm_fwd(_dev(inp["x"]), _dev(inp["keep"]) if keep else None, _dev(inp["h0"]), _dev(inp["c0"]), _dev(inp["w_ih"]),
                                     _dev(inp["w_hh"]), _dev(inp["b_ih"]), _dev(inp["b_hh"]), want_stash=stash,
                                     w_head=_dev(inp["w_head"]) if heads else None, b_head=_dev(inp["b_head"]) if heads else None, heads=hb)
    torch.cuda.synchronize()
    out = {"y": y, "hn": hn, "cn": cn}
    if stash:
        H = y.shape[-1]
        out["stash"] = st if I > 6 or whole_stash else st[..., :5 * H].contiguous()
    if heads:
        out["heads"] = hb
    return out


def want_fwd(inp, keep):
    """the layer in f64 (oracle/ppo_oracle.py lstm_layer_forward's recurrence, env-major, with the stash rows)"""
    d = {k: torch.from_numpy(v).double() for k, v in inp.items()}
    N, T, _ = d["x"].shape
    h, c = d["h0"], d["c0"]
    ys, st = [], []
    for t in range(T):
        if keep:
            k = d["keep"][:, t, None]
            h, c = h * k, c * k
        g = d["x"][:, t] @ d["w_ih"].T + d["b_ih"] + h @ d["w_hh"].T + d["b_hh"]
        i, f, gg, o = g.chunk(4, dim=-1)
        i, f, gg, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(gg), torch.sigmoid(o)
        st.append(torch.cat([i, f, gg, o, c, h], -1))
        c = f * c + i * gg
        h = o * torch.tanh(c)
        ys.append(h)
    y = torch.stack(ys, 1)
    return {"y": y, "hn": h, "cn": c, "stash": torch.stack(st, 1), "heads": y @ d["w_head"].T + d["b_head"]}


# ------------------------------------------------------------------------------------------------ BPTT + weight gradients
BWD_BUFFERS = ("dgates", "dh0", "dc0", "dw_ih", "dw_hh", "db", "dw_head")


def bwd_inputs(H, N, T):
    """fwd_inputs at I = 6 and what drives the backward: head gradients, plain dy, and gradients of the final state"""
    inp = fwd_inputs(H, T, N, 6)
    rs = np.random.RandomState(1000 * H + 10 * T + N + 5)
    inp.update(dheads=(rs.randn(N, T, NHD) * 1e-2).astype(np.float32), dy=(rs.randn(N, T, H) * 1e-2).astype(np.float32),
               dhn=_uni(rs, (N, H), 1e-2), dcn=_uni(rs, (N, H), 1e-2))
    return inp


def run_bwd(inp, drive, arith="fp16x3", tile=False):
    """{dgates (f32 rows), dh0, dc0, dw_ih, dw_hh, db[, dw_head]} of uav_lstm_bwd + uav_lstm_wgrad, driven by dheads + w_head ("heads")
    or by plain dy ("dy"), on the stash and y of run_fwd in the same arithmetic; tile: the gate gradients in tile form"""
    from uavppo import ops
    N, T, I = inp["x"].shape
    f = run_fwd(inp, True, False, True, arith, whole_stash=True)
    H = f["y"].shape[-1]
    by = ({"dheads": _dev(inp["dheads"]), "w_head": _dev(inp["w_head"])} if drive == "heads" else {"dy": _dev(inp["dy"])})
    with ops.lstm_arith(arith):
        dg = None
        if tile:
            dg = ops.lstm_dgates_tile(N, T, I, H, DEV)
            assert dg is not None, ops.lib().uav_last_error()
            dg.fill_(float("nan"))
        try:
            g = ops.lstm_bwd(_dev(inp["x"]), _dev(inp["keep"]), f["stash"], _dev(inp["w_ih"]), _dev(inp["w_hh"]), f["y"], _dev(inp["h0"]),
                             dhn=_dev(inp["dhn"]), dcn=_dev(inp["dcn"]), dgates=dg, dgates_tile=tile, **by)
            g["dgates"] = ops.lstm_dgates_f32(g["dgates"], N, T, H)
        finally:
            if tile:
                ops.lstm_dgates_forget(dg)
    torch.cuda.synchronize()
    return {k: g[k] for k in BWD_BUFFERS if g[k] is not None}


# ------------------------------------------------------------------------------------------------ the cases
def _bwd_case(H, N, T, arith, tile=False):
    def bwd():
        inp = bwd_inputs(H, N, T)
        return {d + "." + k: v for d in (("heads",) if tile else BWD_DRIVES) for k, v in run_bwd(inp, d, arith, tile).items()}
    return bwd


def _fwd_case(H, T, N, combos, arith):
    def fwd():
        out = {}
        for I, s, h, k in combos:
            for name, v in run_fwd(fwd_inputs(H, T, N, I), s, h, k, arith).items():
                out[combo_name(I, s, h, k) + "." + name] = v
        return out
    return fwd


def case_arith(name):
    """the arithmetic a case runs on: its name's suffix, fp16x3 without one"""
    return next((a for a in ARITHS if name.endswith("-" + a)), "fp16x3")


def cases():
    """name -> callable() -> {buffer name: tensor}"""
    c = {}
    for H in (64, 128):
        for N, T in WGRAD_SHAPES:
            for heads in (False, True):
                c["wgrad-h%d-n%d-t%d-%s" % (H, N, T, "heads" if heads else "noheads")] = (
                    lambda H=H, N=N, T=T, hd=heads: run_wgrad(wgrad_inputs(H, N, T), hd))
        for T in FWD_T:
            for N in FWD_N:
                c["fwd-h%d-t%d-n%d" % (H, T, N)] = _fwd_case(H, T, N, fwd_combos(), "fp16x3")
        for N, T in BWD_SHAPES:
            c["bwd-h%d-n%d-t%d-fp16x3" % (H, N, T)] = _bwd_case(H, N, T, "fp16x3")
        for a in ARITHS[:2]:                                                      # the exact-f32 kernels read rows only
            c["bwd-tile-h%d-n%d-t%d-%s" % ((H,) + BWD_TILE_SHAPE + (a,))] = _bwd_case(H, *BWD_TILE_SHAPE, a, tile=True)
        for a in ARITHS[1:]:
            for T in OTHER_FWD_T:
                c["fwd-h%d-t%d-n%d-%s" % (H, T, OTHER_FWD_N, a)] = _fwd_case(H, T, OTHER_FWD_N, OTHER_FWD_COMBOS, a)
            c["bwd-h%d-n%d-t%d-%s" % ((H,) + OTHER_BWD_SHAPE + (a,))] = _bwd_case(H, *OTHER_BWD_SHAPE, a)
            for N, T in OTHER_WGRAD_SHAPES:
                for heads in (False, True):
                    c["wgrad-h%d-n%d-t%d-%s-%s" % (H, N, T, "heads" if heads else "noheads", a)] = (
                        lambda H=H, N=N, T=T, hd=heads, a=a: run_wgrad(wgrad_inputs(H, N, T), hd, a))
    return c


def run_case(name):
    from uavppo import ops
    with ops.lstm_arith(case_arith(name)):
        return {k: _sha(v) for k, v in cases()[name]().items()}


def main():
    out = {}
    for name in cases():
        out[name] = run_case(name)
        assert run_case(name) == out[name], f"{name}: two runs differ"
        print(f"{name}: {len(out[name])} buffers")
    path = sys.argv[1] if len(sys.argv) > 1 else PATH
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{path}: {len(out)} cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
