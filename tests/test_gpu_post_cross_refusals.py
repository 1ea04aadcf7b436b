"""Every refusal of ``post_cross_sq``, ``post_cross_lin_sq`` and ``post_cross_min`` on tiny device operands, word for word and — for
the double faults — in the order of the commit before the three wrappers took one operand-and-window check
(tests/golden/score_refusals.json, section "post_cross", written by tools/score_refusals.py on a GPU).  Nothing is launched: every
case is refused first."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import score_refusal_cases as rc  # noqa: E402

pytestmark = pytest.mark.gpu

with open(rc.GOLDEN) as _f:
    _GOLDEN = json.load(_f)["post_cross"]


def test_the_recorded_cases_are_the_cases():
    assert sorted(_GOLDEN) == sorted(rc.POST_CROSS_CASES)
    assert all(v.startswith("GppError: ") for v in _GOLDEN.values()), _GOLDEN


@pytest.mark.parametrize("name", sorted(rc.POST_CROSS_CASES))
def test_refusal_unchanged(gpu_ctx, name):
    got = rc.record(rc.POST_CROSS_CASES[name])
    print(name, "->", got)
    assert got == _GOLDEN[name]
