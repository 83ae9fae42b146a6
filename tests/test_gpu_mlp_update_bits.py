"""The fused MLP update mlp_ppo_grad_kernel (csrc/mlp_update.hip) against a recording.  The kernel is tuned for registers and its
source gets reshaped for readability; none of that may change a bit of what it writes.
tests/golden/mlp_update_bits.json holds SHA-256 digests of the gradient, the loss sums and the diagnostic sums of every case,
recorded by tools/gen_golden_mlp_update_bits.py on the build before such a change; this build must reproduce each one.  The cases
and what each is chosen for are defined once, in the generator; the oracle for these entry points is held by
tests/test_gpu_trainer.py, test_gpu_trend_mlp.py, test_gpu_inline_update.py and test_gpu_ppo_diag.py.
-m gpu."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gen():
    spec = importlib.util.spec_from_file_location("gen_golden_mlp_update_bits", os.path.join(ROOT, "tools", "gen_golden_mlp_update_bits.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


GEN = _gen()
with open(GEN.PATH) as _f:
    GOLD = json.load(_f)


def test_the_recording_covers_every_case():
    assert sorted(GOLD["cases"]) == sorted(GEN.cases())


@pytest.mark.parametrize("name", sorted(GEN.cases()))
def test_kernel_reproduces_the_recorded_bits(name):
    cus = GEN.cu_count()
    assert cus == GOLD["cu_count"], (f"recorded on {GOLD['cu_count']} CUs, this device has {cus}: the update sums one gradient slab per "
                                     "CU, so the summation order -- and with it the bits -- belong to the CU count")
    digests, want = GEN.run_case(name), GOLD["cases"][name]
    assert sorted(digests) == sorted(want)
    differ = [k for k in sorted(want) if digests[k] != want[k]]
    assert not differ, f"{name}: buffers that differ from the recording: {differ}"
