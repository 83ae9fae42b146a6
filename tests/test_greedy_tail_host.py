"""Host side of the greedy tail route: which of the three evaluation routes the fused= / tail= keywords select
(uavppo.greedy.greedy_route), and that uav_greedy_tail is declared, bound and documented.  No GPU."""
import itertools
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _route(fused, tail, fused_why, tail_why):
    from uavppo.greedy import greedy_route
    return greedy_route(fused, tail, fused_why, tail_why, "evaluate")


@pytest.mark.parametrize("fused,tail", list(itertools.product((None, True, False), repeat=2)))
def test_route_for_every_keyword_combination(fused, tail):
    """All nine (fused, tail) pairs against the four (covered / refused) x (covered / refused) policies."""
    for fused_why, tail_why in itertools.product((None, "no fused kernel"), (None, "no tail route")):
        if fused is True:                                   # the fused kernel or an error, whatever tail says
            want = "fused" if fused_why is None else RuntimeError
        elif tail is True:                                  # the tail route or an error
            want = "tail" if tail_why is None else RuntimeError
        elif fused is None and fused_why is None:
            want = "fused"
        elif fused is None and tail is None and tail_why is None:
            want = "tail"                                   # only where the fused kernel refused
        else:
            want = "stepwise"                               # fused=False alone, tail=False, or nothing covers the policy
        if want is RuntimeError:
            why = fused_why if fused is True else tail_why
            with pytest.raises(RuntimeError, match=re.escape(f"evaluate({'fused' if fused is True else 'tail'}=True): {why}")):
                _route(fused, tail, fused_why, tail_why)
        else:
            assert _route(fused, tail, fused_why, tail_why) == want, (fused, tail, fused_why, tail_why)


def test_the_named_cases_of_the_keywords():
    assert _route(None, None, "h = 256", None) == "tail"            # the default changes route only where the fused kernel refuses
    assert _route(None, None, None, None) == "fused"
    assert _route(False, None, "fused=False", None) == "stepwise"   # fused=False alone still means the step-wise loop
    assert _route(None, False, "h = 256", "tail=False") == "stepwise"
    assert _route(False, True, "fused=False", None) == "tail"
    assert _route(None, None, "an MLP of another size", "an MLP") == "stepwise"


def test_uav_greedy_tail_is_declared_bound_and_documented():
    from uavppo import _lib
    header = open(os.path.join(ROOT, "include", "uavppo.h")).read()
    assert len(re.findall(r"\buav_greedy_tail\b", header)) == 1
    m = re.search(r"int uav_greedy_tail\(([^;]*)\);", header)
    assert m is not None
    n_args = len(m.group(1).split(","))
    binding = open(os.path.join(ROOT, "uav-wrf-les-ppo-lstm_amd", "uavppo", "_lib.py")).read()
    assert len(re.findall(r"\buav_greedy_tail\b", binding)) == 1
    assert len(_lib.SIGNATURES["uav_greedy_tail"][1]) == n_args == 25
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert len(re.findall(r"\buav_greedy_tail\b", doc)) == 1
    from uavppo import ops
    assert callable(ops.greedy_tail)
