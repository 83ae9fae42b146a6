"""The h = 64 / 128 update kernels lstm_fwd_split (csrc/lstm.hip) and lstm_wgrad_split (csrc/wgrad.hip) against a recording and
against f64.  Such kernels are tuned for instruction issue (lstm_wgrad_split: scalar bases + 32-bit offsets instead of per-load
64-bit addresses, unconditional clamped prefetches; the forward's cases stand ready for the same work on its x / keep staging);
none of that may change a bit of what they write.
tests/golden/update_bits.json holds SHA-256 digests of every output buffer, recorded by tools/gen_golden_update_bits.py on the build
before that tuning; this build must reproduce each one.  The same outputs are also held to the rule of tests/test_gpu_lstm.py against
an f64 restatement (error <= 2 x the exact-f32 kernels' error + 2e-7, each relative to the buffer's largest magnitude), so a wrong
address fails even against a regenerated recording.  The cases and what each is chosen for are defined once, in the generator.
-m gpu."""
import functools
import importlib.util
import json
import os

import pytest

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


def _hold_to_the_f32_rule(tag, run, want):
    e_split, e_f32 = _errs(run("fp16x3"), want), _errs(run("f32_mfma"), want)
    for k in e_split:
        print(tag, k, "split %.3e" % e_split[k], "exact f32 %.3e" % e_f32[k])
        assert e_split[k] < 5e-6, (tag, k, e_split[k])
        assert e_split[k] <= 2.0 * e_f32[k] + 2e-7, (tag, k, e_split[k], e_f32[k])


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
