"""Optimisation by the knowledge gradient: the next q runs of a simulator are the candidates whose observation is expected to lower
the minimum of the emulator's posterior mean over a reference set the most (Frazier, Powell & Dayanik 2009; per unit cost in the
multi-fidelity form of Wu & Frazier).  The greedy batch of ``GP_Plus.knowledge_gradient``'s criterion.  No reference counterpart: the
reference's acquisition functions (AFs.py) score a point by the prediction at that point."""
from __future__ import annotations

from typing import Tuple

import torch

__all__ = ["select_by_knowledge_gradient"]


def select_by_knowledge_gradient(model, q: int, Xcand, Xref, cost=None, maximize: bool = False,
                                 num_nodes: int = 32) -> Tuple[torch.Tensor, torch.Tensor]:
    """``q`` rows of ``Xcand`` picked greedily by ``model.knowledge_gradient``'s score over ``Xref`` (with ``cost``, M_c positive
    numbers, by score per unit cost).  Between the picks no value is observed and nothing is factorised: a picked candidate's
    observation is believed to equal its predicted mean (the "Kriging believer" of Ginsbourger et al. 2010), so the mean stays and
    the posterior covariance shrinks as under ``condition_on``.  Returns (indices into ``Xcand`` in pick order, the gains in the
    units of y, undivided by the cost).  The gains of this heuristic, unlike those of ``select_by_variance_reduction``, do not add
    up to a joint quantity.  The score is a ``num_nodes``-point Gauss-Hermite approximation (see ``GP_Plus.knowledge_gradient``).
    A multi-fidelity user passes candidates of several sources, reference rows of the high-fidelity source and the cost of each
    candidate's source.  ``ValueError`` for q < 1 or q > M_c, bad costs and everything ``knowledge_gradient`` refuses.  The loop it
    closes: score -> pick (x, source) -> run -> ``condition_on`` -> score."""
    if int(q) < 1:
        raise ValueError(f"select_by_knowledge_gradient: q must be at least 1 (got {q})")
    _, picks, gains = model._knowledge_gradient(Xcand, Xref, q=int(q), cost=cost, maximize=maximize, num_nodes=num_nodes)
    return picks, gains
