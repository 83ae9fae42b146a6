"""The h = 64 / 128 update kernels lstm_fwd_split (csrc/lstm.hip) and lstm_wgrad_split (csrc/wgrad.hip) against a recording and
against f64.  Such kernels are tuned for instruction issue (lstm_wgrad_split: scalar bases + 32-bit offsets instead of per-load
64-bit addresses, unconditional clamped prefetches; the forward's cases stand ready for the same work on its x / keep staging);
none of that may change a bit of what they write.
tests/golden/update_bits.json holds SHA-256 digests of every output buffer, recorded by tools/gen_golden_update_bits.py on the build
before that tuning; this build must reproduce each one.  The same outputs are also held to the rule of tests/test_gpu_lstm.py against
an f64 restatement (error <= 2 x the exact-f32 kernels' error + 2e-7, each relative to the buffer's largest magnitude), so a wrong
address fails even against a regenerated recording.  The cases and what each is chosen for are defined once, in the generator.
Since the FMAs of lstm.hip / wgrad.hip were written out (they used to be the compiler's choice), the recording also pins the BPTT
(lstm_bwd_split in rows and tile form, the exact-f32 lstm_bwd_kernel) and all three kernel families on bf16x6 and f32_mfma; those
buffers are held to the same rule, the backward against the f64 layer of tests/test_gpu_lstm_arith.py (want_bwd).
-m gpu."""
import functools
import importlib.util
import json
import os

import pytest
import torch

from test_gpu_lstm_arith import oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gen():
    spec = importlib.util.spec_from_file_location("gen_golden_update_bits", os.path.join(ROOT, "tools", "gen_golden_update_bits.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


GEN = _gen()
with open(GEN.PATH) as _f:
    GOLD = json.load(_f)


def test_the_recording_covers_every_case():
    assert sorted(GOLD) == sorted(GEN.cases())


@pytest.mark.parametrize("name", sorted(GEN.cases()))
def test_kernel_reproduces_the_recorded_bits(name):
    digests, want = GEN.run_case(name), GOLD[name]
    assert sorted(digests) == sorted(want)
    differ = [k for k in sorted(want) if digests[k] != want[k]]
    assert not differ, f"{name}: buffers that differ from the recording: {differ}"


def _errs(got, want):
    return {k: float((got[k].detach().cpu().double() - want[k][..., :got[k].shape[-1]]).abs().max() / (want[k].abs().max() + 1e-30)) for k in got}


def _hold_to_the_f32_rule(tag, run, want, splits=("fp16x3",)):
    e_f32 = _errs(run("f32_mfma"), want)
    for split in splits:
        e_split = _errs(run(split), want)
        for k in e_split:
            print(tag, k, split, "%.3e" % e_split[k], "exact f32 %.3e" % e_f32[k])
            assert e_f32[k] < 5e-6, (tag, k, e_f32[k])
            assert e_split[k] < 5e-6, (tag, split, k, e_split[k])
            assert e_split[k] <= 2.0 * e_f32[k] + 2e-7, (tag, split, k, e_split[k], e_f32[k])


@pytest.mark.parametrize("heads", [False, True], ids=["noheads", "heads"])
@pytest.mark.parametrize("N,T", GEN.WGRAD_SHAPES)
@pytest.mark.parametrize("H", [64, 128])
def test_weight_gradients_against_f64(H, N, T, heads):
    inp = GEN.wgrad_inputs(H, N, T)
    _hold_to_the_f32_rule((H, N, T, heads), lambda arith: GEN.run_wgrad(inp, heads, arith), GEN.want_wgrad(inp, heads))


@pytest.mark.parametrize("N", GEN.FWD_N)
@pytest.mark.parametrize("T", GEN.FWD_T)
@pytest.mark.parametrize("H", [64, 128])
def test_forward_against_f64(H, T, N):
    inputs = functools.lru_cache(None)(lambda I: GEN.fwd_inputs(H, T, N, I))
    want = functools.lru_cache(None)(lambda I, keep: GEN.want_fwd(inputs(I), keep))
    for I, stash, heads, keep in GEN.fwd_combos():
        _hold_to_the_f32_rule((H, T, N, GEN.combo_name(I, stash, heads, keep)),
                              lambda arith: GEN.run_fwd(inputs(I), stash, heads, keep, arith), want(I, keep))


@pytest.mark.parametrize("heads", [False, True], ids=["noheads", "heads"])
@pytest.mark.parametrize("N,T", GEN.OTHER_WGRAD_SHAPES)
@pytest.mark.parametrize("H", [64, 128])
def test_weight_gradients_on_bf16x6_against_f64(H, N, T, heads):
    inp = GEN.wgrad_inputs(H, N, T)
    _hold_to_the_f32_rule((H, N, T, heads), lambda arith: GEN.run_wgrad(inp, heads, arith), GEN.want_wgrad(inp, heads), ("bf16x6",))


@pytest.mark.parametrize("T", GEN.OTHER_FWD_T)
@pytest.mark.parametrize("H", [64, 128])
def test_forward_on_bf16x6_against_f64(H, T):
    N = GEN.OTHER_FWD_N
    for I, stash, heads, keep in GEN.OTHER_FWD_COMBOS:
        inp = GEN.fwd_inputs(H, T, N, I)
        _hold_to_the_f32_rule((H, T, N, GEN.combo_name(I, stash, heads, keep)),
                              lambda arith: GEN.run_fwd(inp, stash, heads, keep, arith), GEN.want_fwd(inp, keep), ("bf16x6",))


def want_bwd(inp, drive):
    """The recorded backward buffers from the f64 layer of tests/test_gpu_lstm_arith.py (forward + autograd).  The gate gradients are
    that layer's dx of 4H further inputs, all zero, each wired to one gate through an identity block appended to w_ih."""
    d = {k: torch.from_numpy(v).double() for k, v in inp.items()}
    N, T, I = d["x"].shape
    G = d["w_ih"].shape[0]
    tm = lambda t: t.transpose(0, 1)                                             # noqa: E731  env-major -> the oracle's time-major
    p = {k: d[k] for k in ("h0", "c0", "w_hh", "b_ih", "b_hh", "w_head", "b_head", "dhn", "dcn")}
    p.update(x=torch.cat([tm(d["x"]), torch.zeros(T, N, G, dtype=torch.float64)], -1),
             w_ih=torch.cat([d["w_ih"], torch.eye(G, dtype=torch.float64)], 1), keep=tm(d["keep"]))
    p["dheads" if drive == "heads" else "dy"] = tm(d["dheads" if drive == "heads" else "dy"])
    w = oracle(p)
    out = {"dgates": w["dx"][..., I:], "dw_ih": w["dw_ih"][:, :I]}
    out.update({k: w[k] for k in ("dh0", "dc0", "dw_hh", "db") + (("dw_head",) if drive == "heads" else ())})
    return out


@pytest.mark.parametrize("drive", GEN.BWD_DRIVES)
@pytest.mark.parametrize("N,T", GEN.BWD_SHAPES + (GEN.BWD_TILE_SHAPE,))
@pytest.mark.parametrize("H", [64, 128])
def test_bptt_against_f64(H, N, T, drive):
    """both split arithmetics at every recorded shape; at the tile shape the split BPTT writes tile form (the exact kernels read rows)"""
    inp = GEN.bwd_inputs(H, N, T)
    tile = (N, T) == GEN.BWD_TILE_SHAPE and drive == "heads"
    _hold_to_the_f32_rule((H, N, T, drive), lambda arith: GEN.run_bwd(inp, drive, arith, tile and arith != "f32_mfma"),
                          want_bwd(inp, drive), ("fp16x3", "bf16x6"))
