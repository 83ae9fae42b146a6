"""The source-estimate kernels (csrc/source_fit.hip, csrc/source_aniso.hip; one body for both in csrc/source_core.h and
csrc/source_solve.h) against a recording.  tests/golden/source_bits.json holds SHA-256 digests of every output buffer, whole --
states, estimates (peak and strength too), statuses, sums, per-env errors, the stop scan's state, hits, per-record outputs and
marked flags -- recorded by tools/gen_golden_source_bits.py on the build before the kernels were given one body; this build must
reproduce each one.  A digest that differs is an operand order that moved, not a tolerance question.  The cases and what each is
chosen for are defined once, in the generator; what the buffers must BE is asserted against the numpy statement in
tests/test_gpu_source_fit.py, test_gpu_source_aniso.py and test_gpu_source_stop.py.
-m gpu."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gen():
    spec = importlib.util.spec_from_file_location("gen_golden_source_bits", os.path.join(ROOT, "tools", "gen_golden_source_bits.py"))
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
