"""Every argument error of the candidate scores (``variance_reduction`` with and without ``gradient=``, ``knowledge_gradient``, the
three ``select_*`` drivers), of ``active_subspace`` and of ``condition_on`` on two CPU models, word for word and — for the double
faults — in the order of the commit before the scores took one host path (tests/golden/score_refusals.json, section "host", written
by tools/score_refusals.py); a valid call of each ends at the missing device."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import score_refusal_cases as rc  # noqa: E402

with open(rc.GOLDEN) as _f:
    _GOLDEN = json.load(_f)["host"]


def test_the_recorded_cases_are_the_cases():
    assert sorted(_GOLDEN) == sorted(rc.HOST_CASES)


def test_a_valid_call_of_every_method_ends_at_the_missing_device():
    valid = [n for n in rc.HOST_CASES if n.endswith(": valid")]
    assert len(valid) == 8
    for n in valid:
        assert _GOLDEN[n].startswith("GppError: ") and "no CPU fallback" in _GOLDEN[n], (n, _GOLDEN[n])


def test_check_explains_a_missing_workspace():
    from gpplus_amd import _lib, backend

    assert backend.NO_WORKSPACE == _lib.NO_WORKSPACE == 2002
    with pytest.raises(_lib.GppError) as e:
        _lib.check(2002, "x")
    assert str(e.value) == "x: the handle's scratch workspace is missing or too small"


@pytest.mark.parametrize("name", sorted(rc.HOST_CASES))
def test_refusal_unchanged(name):
    got = rc.record(rc.HOST_CASES[name])
    print(name, "->", got)
    assert got == _GOLDEN[name]
