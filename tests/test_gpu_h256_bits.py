"""The h = 256 fp16-split step path (csrc/lstm_h3.hip: sequence forward, stepper, BPTT, the pipelined BPTT of a stack, with the
weight-gradient pass of csrc/wgrad_pc.hip behind it) against a recording.  Its host side -- workspace layout, preparation launches,
step dispatch -- and its kernels get reworked and tuned; none of that may change a bit of what the path writes.
tests/golden/h256_bits.json holds SHA-256 digests of every output buffer, recorded by tools/gen_golden_h256_bits.py on the build
before the host side was given one layout, one prologue and one step launcher; this build must reproduce each one.  Accuracy against
f64 is the business of tests/test_gpu_lstm_h256.py and tests/test_gpu_lstm.py.  The cases and what each is chosen for are defined
once, in the generator.  -m gpu."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gen():
    spec = importlib.util.spec_from_file_location("gen_golden_h256_bits", os.path.join(ROOT, "tools", "gen_golden_h256_bits.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


GEN = _gen()
with open(GEN.PATH) as _f:
    GOLD = json.load(_f)


def test_the_recording_covers_every_case():
    assert sorted(GOLD) == sorted(GEN.cases())


@pytest.mark.parametrize("name", sorted(GEN.cases()))
def test_step_path_reproduces_the_recorded_bits(name):
    digests, want = GEN.run_case(name), GOLD[name]
    assert sorted(digests) == sorted(want)
    differ = [k for k in sorted(want) if digests[k] != want[k]]
    assert not differ, f"{name}: buffers that differ from the recording: {differ}"
