"""The value and every gradient of each training objective, eager and batched, bit for bit against the digests recorded from the
commit before the objectives took one host scaffold (tests/golden/objective_bits.json, written by tools/objective_bits.py): a
rearrangement of the host code around the launches changes no launch, no operand and no order of additions."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import objective_bits_cases as oc  # noqa: E402

pytestmark = pytest.mark.gpu

with open(oc.GOLDEN) as _f:
    _GOLDEN = json.load(_f)


def test_the_recorded_cases_are_the_cases():
    assert sorted(_GOLDEN["cases"]) == sorted(oc.CASES)


@pytest.mark.parametrize("name", sorted(oc.CASES))
def test_objective_bits_unchanged(gpu_ctx, name):
    assert oc.source_hash() == _GOLDEN["library_source"], (
        f"the library's sources ({oc.source_hash()}) are not those the digests were recorded from ({_GOLDEN['library_source']}): "
        "regenerate tests/golden/objective_bits.json with tools/objective_bits.py only for a deliberate change of arithmetic")
    got = oc.digests(oc.CASES[name])
    print(name, {k: v[:12] for k, v in got.items()})
    assert got == _GOLDEN["cases"][name]
