"""Bit-identity of the policy-step kernels against a recording: rollout_lstm_kernel, rollout_mlp_kernel, rollout_tail_kernel,
greedy_tail_kernel and env_step_kernel share their per-env arithmetic (argmax, the fused draw, noise -> wind -> step, auto-reset,
flags, the greedy record) through the core headers of csrc/, so the route-against-route identities of the other test files cannot
see a mistake made there -- every route would make it.  tests/golden/step_bits.json holds SHA-256 digests of every output buffer
and of the env state blob of each route, recorded by tools/gen_golden_step_bits.py on the build before that code was shared; this
build must reproduce each one.  The cases, their inputs and the branches a run must walk are defined once, in the generator.
-m gpu."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gen():
    spec = importlib.util.spec_from_file_location("gen_golden_step_bits", os.path.join(ROOT, "tools", "gen_golden_step_bits.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


GEN = _gen()
with open(GEN.PATH) as _f:
    GOLD = json.load(_f)


def test_the_recording_covers_every_case():
    assert sorted(GOLD) == sorted(GEN.cases())


@pytest.mark.parametrize("name", sorted(GEN.cases()))
def test_route_reproduces_the_recorded_bits(name):
    digests, facts = GEN.run_case(name, GOLD[name]["seed"])
    # the run walked what the recording was chosen for: an auto-reset before the last step of a training rollout; in a greedy
    # run an episode ended by `done`, one ended by the rule's hit where there is a rule, and an env still active at the end
    assert all(facts.values()), facts
    want = GOLD[name]["sha256"]
    assert sorted(digests) == sorted(want)
    differ = [k for k in sorted(want) if digests[k] != want[k]]
    assert not differ, f"{name}: buffers that differ from the recording: {differ}"
