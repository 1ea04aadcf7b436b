"""Active learning by expected variance reduction: the next q runs of a simulator are the candidates whose observation most reduces
the emulator's posterior variance over a reference set (Cohn 1996, "ALC"; integrated mean squared error over the reference set).
The greedy batch of ``GP_Plus.variance_reduction``'s criterion.  No reference counterpart: the reference's acquisition functions
(AFs.py) serve optimisation, and scoring by refit costs a factorisation per candidate."""
from __future__ import annotations

from typing import Tuple

import torch

__all__ = ["select_by_variance_reduction"]


def select_by_variance_reduction(model, q: int, Xcand, Xref, weights=None, cost=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``q`` rows of ``Xcand`` picked greedily: each round takes the candidate with the largest expected reduction of the weighted
    posterior variance over ``Xref`` given the picks so far (with ``cost``, M_c positive numbers, the largest reduction per unit
    cost), then accounts for it — no value is observed and nothing is factorised, the posterior variance does not depend on the
    values.  Returns (indices into ``Xcand`` in pick order, the gains in y^2 units, undivided by the cost); the gains add up to the
    reduction ``model.condition_on`` of all q picks would give.  A multi-fidelity user passes candidates of several sources,
    reference rows of the high-fidelity source and the cost of each candidate's source.  ``ValueError`` for q < 1 or q > M_c and
    for everything ``variance_reduction`` refuses.  The loop it closes: score -> pick -> run -> ``condition_on`` -> score."""
    if int(q) < 1:
        raise ValueError(f"select_by_variance_reduction: q must be at least 1 (got {q})")
    _, picks, gains = model._variance_reduction(Xcand, Xref, weights, q=int(q), cost=cost)
    return picks, gains
