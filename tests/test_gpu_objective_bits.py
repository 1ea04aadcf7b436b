"""Bit for bit against digests recorded from the commit before a rearrangement of the host code (written by tools/objective_bits.py):
the value and every gradient of each training objective, eager and batched (tests/golden/objective_bits.json, from the commit before
the objectives took one host scaffold), and every candidate score at the ``linalg`` and the model level (tests/golden/score_bits.json,
from the commit before the scores took one host path).  A rearrangement of the host code around the launches changes no launch, no
operand and no order of additions."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import objective_bits_cases as oc  # noqa: E402
import score_bits_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu


def _golden(mod):
    with open(mod.GOLDEN) as f:
        return json.load(f)


_GOLDEN = {mod: _golden(mod) for mod in (oc, sc)}
#: (module, case): the objectives under their bare names, the scores behind "score-"
_PARAMS = [pytest.param(oc, n, id=n) for n in sorted(oc.CASES)] + [pytest.param(sc, n, id="score-" + n) for n in sorted(sc.CASES)]


def test_the_recorded_cases_are_the_cases():
    for mod, golden in _GOLDEN.items():
        assert sorted(golden["cases"]) == sorted(mod.CASES)


@pytest.mark.parametrize("mod,name", _PARAMS)
def test_objective_bits_unchanged(gpu_ctx, mod, name):
    golden = _GOLDEN[mod]
    assert mod.source_hash() == golden["library_source"], (
        f"the library's sources ({mod.source_hash()}) are not those the digests were recorded from ({golden['library_source']}): "
        f"regenerate {os.path.basename(mod.GOLDEN)} with tools/objective_bits.py only for a deliberate change of arithmetic")
    got = mod.digests(mod.CASES[name])
    print(name, {k: v[:12] for k, v in got.items()})
    assert got == golden["cases"][name]
